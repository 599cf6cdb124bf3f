#!/usr/bin/env python3
"""Host emit vs the opt-in device emit (SPX_DEVICE_EMIT=1) on the tier-3 input: one
synthetic clustered MGF (synthetic.write_clustered_mgf, the file tools/bench_ingest.py
reads).

Per CLI that has the switch (binning, gap-average), in one process, both arms on the
SAME device-resident result, alternating, median of --runs (>= 5) runs with every run
listed (the spread):

* baseline arm, the path without the switch: the peaks' D2H (``to_host()``), then
  formatting plus write (``mgf_native.write_records``);
* device arm: the small readback, compaction, the format kernels, the text's D2H and
  the header-and-splice write, each ending in a device synchronise;
* the format kernels alone on preallocated buffers, as GB/s of text;
* each CLI end to end with the switch unset and set, with and without
  SPX_DEVICE_INGEST=1.

Every pair of outputs is compared byte for byte.  Prints one JSON line and, with
--out, writes it to a file.

    python tools/bench_emit.py [--clusters 20000] [--runs 5] [--tmpdir DIR] [--out FILE] [--skip-clis]
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-clis", action="store_true")
    ap.add_argument("--only", default=None, help="one leg: binning or average_spectrum_clustering")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5 (medians)")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_emit.py needs a HIP device")
    from specpride_amd import average_spectrum_clustering as asc
    from specpride_amd import binning, device_emit, device_ingest, engine, mgf_native
    from specpride_amd.synthetic import write_clustered_mgf

    def sync():
        torch.cuda.synchronize()

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    def med(xs):
        return round(statistics.median(xs), 4)

    def same(a, b):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            return fa.read() == fb.read()

    # ---- per CLI: (device result, baseline arm, device arm), both arms writing the same records
    def binning_leg(path):
        batch, meta = device_ingest.load(path, False, mgf_native.GROUP_BINNING)
        res = engine.bin_mean(batch)
        style, ids = mgf_native.STYLE_BINNING, meta["ids"]

        def base(out, st):
            t0 = time.perf_counter()
            r = res.to_host()
            sync()
            t1 = time.perf_counter()
            mgf_native.write_records(out, style, ids, r["out_off"], r["out_mz"], r["out_int"], r["prec"], r["charge"])
            st.update(peaks_d2h=t1 - t0, format_and_write=time.perf_counter() - t1)

        return base, lambda out, st: device_emit.write_consensus(out, style, ids, res, binning._raise_for, stages=st)

    def gap_leg(path):
        batch, meta = device_ingest.load(path, True, mgf_native.GROUP_RUNS)
        res = engine.gap_average(batch)
        style, ids = mgf_native.STYLE_GAP_AVERAGE, meta["ids"]

        def base(out, st):
            t0 = time.perf_counter()
            r = res.to_host()
            sync()
            t1 = time.perf_counter()
            mgf_native.write_records(out, style, ids, r["out_off"], r["out_mz"], r["out_int"], r["prec"], r["charge"],
                                     r["rt"])
            st.update(peaks_d2h=t1 - t0, format_and_write=time.perf_counter() - t1)

        return base, lambda out, st: device_emit.write_consensus(out, style, ids, res, asc._raise_for, stages=st)

    legs = {"binning": binning_leg, "average_spectrum_clustering": gap_leg}
    clis = {"binning": lambda i, o: binning.main(["--mgf_file", i, "--out", o]),
            "average_spectrum_clustering": lambda i, o: asc.main([i, o, "--encodedclusters"])}

    for env in (device_emit.ENV, device_ingest.ENV):
        os.environ.pop(env, None)
    out = {"runs": args.runs}
    with tempfile.TemporaryDirectory(dir=args.tmpdir) as td:
        warm, mgf_in = os.path.join(td, "w.mgf"), os.path.join(td, "in.mgf")
        write_clustered_mgf(warm, 200, args.seed + 1)
        S, P = write_clustered_mgf(mgf_in, args.clusters, args.seed)
        out.update(clusters=args.clusters, spectra=S, peaks=P, mgf_in_GB=round(os.path.getsize(mgf_in) / 1e9, 3))
        o_base, o_dev = os.path.join(td, "base.mgf"), os.path.join(td, "dev.mgf")
        for name, make in legs.items():
            if args.only and name != args.only:
                continue
            for arm in make(warm):  # code objects, allocator, staging pool
                arm(o_base, {})
            base, dev = make(mgf_in)
            tb, tdv, sb, sd = [], [], [], []
            for _ in range(args.runs):  # alternating arms
                st = {}
                tb.append(timed(lambda: base(o_base, st)))
                sb.append(st)
                st = {}
                tdv.append(timed(lambda: dev(o_dev, st)))
                sd.append(st)
            out_bytes = os.path.getsize(o_base)
            leg = {"out_GB": round(out_bytes / 1e9, 3), "outputs_identical": same(o_base, o_dev),
                   "host_emit_s": med(tb), "device_emit_s": med(tdv),
                   "host_emit_all_s": [round(x, 4) for x in tb], "device_emit_all_s": [round(x, 4) for x in tdv],
                   "speedup": round(statistics.median(tb) / statistics.median(tdv), 2),
                   "host_stages_s": {k: med([s.get(k, 0.0) for s in sb]) for k in ("peaks_d2h", "format_and_write")},
                   "device_stages_s": {k: med([s.get(k, 0.0) for s in sd]) for k in device_emit.STAGES}}
            spread = max(max(tb) - min(tb), max(tdv) - min(tdv))
            leg["spread_s"] = round(spread, 4)
            leg["device_faster_beyond_spread"] = bool(statistics.median(tb) - statistics.median(tdv) > spread)
            leg["device_bound_by"] = max(leg["device_stages_s"], key=leg["device_stages_s"].get)
            out[name] = leg
            print(json.dumps({name: leg}), file=sys.stderr, flush=True)
            del base, dev
            if args.skip_clis:
                continue
            cli = {}
            with contextlib.redirect_stdout(io.StringIO()):
                for ingest in (False, True):
                    times = {False: [], True: []}
                    outs = {False: os.path.join(td, "cli_off.mgf"), True: os.path.join(td, "cli_on.mgf")}
                    for r in range(args.runs + 1):  # run 0 warms the path up (on the small file)
                        for emit in (False, True):
                            for env, on in ((device_ingest.ENV, ingest), (device_emit.ENV, emit)):
                                os.environ.pop(env, None)
                                if on:
                                    os.environ[env] = "1"
                            dt = timed(lambda: clis[name](warm if r == 0 else mgf_in, outs[emit]))
                            if r:
                                times[emit].append(dt)
                    key = "device_ingest" if ingest else "host_ingest"
                    cli[key] = {"host_emit_s": med(times[False]), "device_emit_s": med(times[True]),
                                "host_emit_all_s": [round(x, 4) for x in times[False]],
                                "device_emit_all_s": [round(x, 4) for x in times[True]],
                                "speedup": round(statistics.median(times[False]) / statistics.median(times[True]), 2),
                                "outputs_identical": same(outs[False], outs[True])}
            for env in (device_emit.ENV, device_ingest.ENV):
                os.environ.pop(env, None)
            leg["cli"] = cli
            print(json.dumps({name + "_cli": cli}), file=sys.stderr, flush=True)
        # ---- the format kernels alone: the binning CLI's consensus peaks, buffers preallocated
        if not args.only or args.only == "binning":
            batch, _meta = device_ingest.load(mgf_in, False, mgf_native.GROUP_BINNING)
            res = engine.bin_mean(batch)
            out_off, dmz, dint = res.compact()
            sb_, se_ = out_off[:-1].contiguous(), out_off[1:].contiguous()
            fr = engine.format_peaks(dmz, dint, sb_, se_, skip_nan=True)
            text_bytes = int(fr.to_host()["text_off"][-1])
            tk = [timed(lambda: engine.format_peaks(dmz, dint, sb_, se_, skip_nan=True, out=fr))
                  for _ in range(args.runs)]
            out["format_kernels"] = {"peaks": int(dmz.numel()), "segments": int(sb_.numel()), "text_bytes": text_bytes,
                                     "all_s": [round(x, 6) for x in tk], "median_s": round(statistics.median(tk), 6),
                                     "text_GBs": round(text_bytes / statistics.median(tk) / 1e9, 2),
                                     "input_GBs": round(16 * dmz.numel() / statistics.median(tk) / 1e9, 2)}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
