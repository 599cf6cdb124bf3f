#!/usr/bin/env python3
"""Explained b/y intensity (spx_by_fraction) over every member spectrum of the configs[1]
batch, inputs resident in HBM, HIP-event timing per call: warm-up, repeated calls, median
with min and max.  Prints one JSON line.

Every cluster gets one random valid peptide of length U{7..30}; its spectra are scored
against it at the cluster's charge (the synthetic spectra are not that peptide's, so few
windows hold a peak: the work is the passes and the searches, as for a real file's
non-matching fragments).

Algorithmic bytes: 16 B per peak (m/z + intensity, read once); the fraction of the
8 TB/s HBM peak that this rate is says how far from memory-bound the call runs.

CPU figure (--cpu-sample N, --cpu-only to run nothing else): the numpy restatement of
tests/by_fraction_cases.py on the first N spectra of the host generator's batch of the same
law with peptides of the same law, 1 core.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RESIDUES = "QWERTYIPASDFGHKLCVNM"


def peptides(n, seed):
    """(bytes back to back, offsets [n + 1]) of n random valid peptides of length U{7..30}."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(7, 31, size=n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    letters = np.frombuffer(RESIDUES.encode(), np.uint8)
    return letters[rng.integers(0, len(letters), size=int(off[-1]))], off


def cpu_figure(n_spectra, seed=0):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import by_fraction_cases as cases
    from specpride_amd.synthetic import make_clusters_np

    csr = make_clusters_np(max(8, n_spectra // 8), seed=seed)
    n_spectra = min(n_spectra, csr.n_spectra)
    seq, off = peptides(csr.n_clusters, seed + 1)
    owner = np.repeat(np.arange(csr.n_clusters), np.diff(csr.cluster_off))
    t0 = time.perf_counter()
    peaks = 0
    for s in range(n_spectra):
        c = owner[s]
        b, e = csr.spec_off[s], csr.spec_off[s + 1]
        cases.restate(bytes(seq[off[c]:off[c + 1]]).decode(), float(csr.prec_mz[s]), int(csr.charge[s]), csr.mz[b:e],
                      csr.inten[b:e])
        peaks += e - b
    dt = time.perf_counter() - t0
    return {"value": round(n_spectra / dt, 2), "unit": "spectra/s", "cores": 1, "kind": "port",
            "sample": f"the first {n_spectra} spectra ({int(peaks)} peaks) of a configs[1]-law batch, numpy "
                      f"restatement of fraction_of_by, {dt:.2f} s"}


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-sample", type=int, default=0, help="spectra timed on 1 host core (0: skip)")
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    if args.cpu_only:
        print(json.dumps({"cpu_baseline": cpu_figure(args.cpu_sample or 2000)}), flush=True)
        return
    import torch

    from specpride_amd import engine
    from specpride_amd.synthetic import make_clusters_torch

    b = engine.DeviceBatch.from_device(make_clusters_torch(args.clusters, seed=0))
    C, S, P = b.n_clusters, b.n_spectra, b.n_peaks
    dev = b.device
    seq, off = peptides(C, 1)
    sizes = np.diff(b.host_cluster_off)
    lens = np.repeat(np.diff(off), sizes)
    seq_off = np.zeros(S + 1, np.int64)
    np.cumsum(lens, out=seq_off[1:])
    # every spectrum carries its cluster's peptide: gather the letters per spectrum
    src = np.repeat(off[:-1], sizes)
    idx = np.repeat(src - seq_off[:-1], lens) + np.arange(int(seq_off[-1]))
    t_seq = torch.as_tensor(seq[idx].copy(), device=dev)
    t_seq_off = torch.as_tensor(seq_off, device=dev)
    so = b.t["spec_off"]
    seg_begin, seg_end = so[:-1].contiguous(), so[1:].contiguous()
    call = lambda out=None: engine.by_fraction(b.t["mz"], b.t["inten"], seg_begin, seg_end, b.t["prec_mz"],  # noqa: E731
                                               b.t["charge"], t_seq, t_seq_off, out=out)
    res = call()
    for _ in range(args.warmup):
        call(res)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        call(res)
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    new = spread(ms)
    nbytes = 16 * P
    gbs = nbytes / (new["median_ms"] * 1e-3) / 1e9
    frac = res.fraction[:S]
    out = {"workload": "configs[1] batch: fraction_of_by of every member spectrum against its cluster's peptide",
           "clusters": C, "spectra": S, "peaks": P, "fragments": int((2 * (lens - 1)
                                                                      * np.maximum(1, b.t["charge"].cpu().numpy() - 1)).sum()),
           "by_fraction": new, "spectra_per_s": round(S / (new["median_ms"] * 1e-3), 1),
           "algorithmic_bytes": nbytes, "algorithmic_GBs": round(gbs, 1),
           "fraction_of_8TBs_peak": round(gbs / 8000.0, 4),
           "status_ok": int((res.status[:S] == 0).sum().item()),
           "mean_fraction": float(frac.mean().item()), "nonzero_fractions": int((frac > 0).sum().item())}
    if args.cpu_sample > 0:
        out["cpu_baseline"] = cpu_figure(args.cpu_sample)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
