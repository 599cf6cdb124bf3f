#!/usr/bin/env python3
"""Host ingest vs the opt-in device ingest (SPX_DEVICE_INGEST=1) on the tier-3
input: one synthetic clustered MGF (synthetic.write_clustered_mgf, the file the
tier-3 leg of bench.py / tools/bench_tiers.py writes).

For each CLI's grammar and grouping, in one process on the same file with a warm
page cache, the two arms alternating, median of --runs (>= 5) runs each:

* ingest up to "DeviceBatch ready": the host path as the CLI runs it without the
  switch (native parse -> grouping -> CSR -> H2D) against device_ingest.load;
* the device path's stages (index, grouping, H2D, kernels, status readback,
  patching, batch), each ending in a device synchronise, from runs of their own;
* each CLI end to end (MGF text in, MGF text out) with the switch unset and set;
  the two outputs are compared byte for byte.

The comparison is always against the host-ingest path, never against the device
path itself.  Prints one JSON line.

    python tools/bench_ingest.py [--clusters 20000] [--runs 5] [--tmpdir DIR] [--skip-clis]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tmpdir", default=None)
    ap.add_argument("--seed", type=int, default=6)
    ap.add_argument("--skip-clis", action="store_true")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5 (medians)")
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_ingest.py needs a HIP device")
    from specpride_amd import average_spectrum_clustering as asc
    from specpride_amd import binning, device_ingest, engine, ingest, mgf_native
    from specpride_amd import most_similar_representative as msr
    from specpride_amd.synthetic import write_clustered_mgf

    def host_binning(path):
        ids, csr = binning._flat_clusters(path)
        return engine.DeviceBatch.from_host(csr)

    def host_runs(path):
        ids, csr = asc._native_runs(path)
        return engine.DeviceBatch.from_host(csr)

    def host_first_runs(path):  # most_similar_representative._main_native up to the batch
        flat = mgf_native.parse_general(path, group=mgf_native.GROUP_FIRST_RUNS)
        key, ids = flat["key"], flat["group_ids"]
        records = np.flatnonzero(key >= 0)
        sizes = np.bincount(key[records], minlength=len(ids))
        return engine.DeviceBatch.from_host(
            ingest.csr_from_flat(flat, sizes, None if len(records) == len(key) else records))

    legs = {"binning": (host_binning, False, mgf_native.GROUP_BINNING),
            "average_spectrum_clustering": (host_runs, True, mgf_native.GROUP_RUNS),
            "most_similar_representative": (host_first_runs, True, mgf_native.GROUP_FIRST_RUNS)}
    clis = {"binning": lambda i, o: binning.main(["--mgf_file", i, "--out", o]),
            "average_spectrum_clustering": lambda i, o: asc.main([i, o, "--encodedclusters"]),
            "most_similar_representative": lambda i, o: msr.main(["-i", i, "-o", o])}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del r
        return dt

    def med(xs):
        return round(statistics.median(xs), 4)

    os.environ.pop(device_ingest.ENV, None)
    out = {"runs": args.runs}
    with tempfile.TemporaryDirectory(dir=args.tmpdir) as td:
        warm, mgf_in = os.path.join(td, "w.mgf"), os.path.join(td, "in.mgf")
        write_clustered_mgf(warm, 200, args.seed + 1)
        S, P = write_clustered_mgf(mgf_in, args.clusters, args.seed)
        size = os.path.getsize(mgf_in)
        out.update(clusters=args.clusters, spectra=S, peaks=P, mgf_GB=round(size / 1e9, 3))
        for name, (host, general, mode) in legs.items():
            dev = lambda p: device_ingest.load(p, general, mode)  # noqa: E731
            assert dev(warm) is not None
            host(warm)  # code objects, allocator, staging pool, page cache
            th, td_ = [], []
            for _ in range(args.runs):  # alternating arms
                th.append(timed(lambda: host(mgf_in)))
                td_.append(timed(lambda: dev(mgf_in)))
            stages, n_reparse = [], 0
            for _ in range(args.runs):
                st = {}
                batch, meta = device_ingest.load(mgf_in, general, mode, stages=st)
                n_reparse = meta["n_reparse"]
                del batch
                stages.append(st)
            leg = {"host_ingest_s": med(th), "device_ingest_s": med(td_),
                   "host_ingest_all_s": [round(x, 4) for x in th], "device_ingest_all_s": [round(x, 4) for x in td_],
                   "host_GBs": round(size / statistics.median(th) / 1e9, 2),
                   "device_GBs": round(size / statistics.median(td_) / 1e9, 2),
                   "speedup": round(statistics.median(th) / statistics.median(td_), 2),
                   "stages_s": {k: med([s.get(k, 0.0) for s in stages]) for k in device_ingest.STAGES},
                   "n_reparse": n_reparse}
            leg["bound_by"] = max(leg["stages_s"], key=leg["stages_s"].get)
            out[name] = leg
            print(json.dumps({name: leg}), file=sys.stderr, flush=True)
            if args.skip_clis:
                continue
            o_off, o_on = os.path.join(td, "off.mgf"), os.path.join(td, "on.mgf")
            c_off, c_on = [], []
            with contextlib.redirect_stdout(io.StringIO()):
                clis[name](warm, o_off)
                for _ in range(args.runs):
                    os.environ.pop(device_ingest.ENV, None)
                    c_off.append(timed(lambda: clis[name](mgf_in, o_off)))
                    os.environ[device_ingest.ENV] = "1"
                    c_on.append(timed(lambda: clis[name](mgf_in, o_on)))
                os.environ.pop(device_ingest.ENV, None)
            with open(o_off, "rb") as a, open(o_on, "rb") as b:
                same = a.read() == b.read()
            leg.update(cli_host_s=med(c_off), cli_device_s=med(c_on),
                       cli_speedup=round(statistics.median(c_off) / statistics.median(c_on), 2),
                       cli_host_clusters_per_s=round(args.clusters / statistics.median(c_off), 1),
                       cli_device_clusters_per_s=round(args.clusters / statistics.median(c_on), 1),
                       cli_outputs_identical=same)
            print(json.dumps({name + "_cli": {k: v for k, v in leg.items() if k.startswith("cli_")}}),
                  file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
