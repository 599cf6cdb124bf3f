#!/usr/bin/env python3
"""Cosine medoid (spx_cosine_medoid) on the configs[1] batch, inputs resident in HBM,
HIP-event timing per call: warm-up, repeated calls, median and spread.  Prints one JSON
line.

Baseline: the only route without the entry point -- for k = 0..max_n-1 one
engine.binned_cosine call with member min(k, n_c - 1) as cluster c's representative
(only the calls are timed, not the gathers that build the representatives); the sum
of the max_n calls is one baseline sample.  Its averages are also compared with the
new scores (member k of every cluster with more than k members).

Algorithmic bytes: 16 B per input peak + 8 B per spectrum out (the scores).

CPU figure (--cpu-sample N, --cpu-only to run nothing else): the reference's
composition -- average_cos_dist(member, members) for every member, restated in
oracle/np_oracle.py -- on the first N clusters of the host generator's batch of the
same law, 1 core.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cpu_figure(n_clusters, seed=0):
    from oracle import np_oracle
    from specpride_amd.synthetic import make_clusters_np

    csr = make_clusters_np(n_clusters, seed=seed)
    t0 = time.perf_counter()
    pairs = 0
    for c in range(csr.n_clusters):
        members = [(csr.mz[csr.spec_off[s]:csr.spec_off[s + 1]], csr.inten[csr.spec_off[s]:csr.spec_off[s + 1]])
                   for s in range(csr.cluster_off[c], csr.cluster_off[c + 1])]
        scores = [np_oracle.average_cos_dist(m, i, members) for m, i in members]
        best = 0
        for k in range(1, len(scores)):
            if scores[k] > scores[best]:
                best = k
        pairs += len(members) ** 2
    dt = time.perf_counter() - t0
    return {"value": round(n_clusters / dt, 4), "unit": "clusters/s", "cores": 1, "kind": "port",
            "sample": f"{n_clusters} clusters of the configs[1] law ({csr.n_spectra} spectra, {pairs} cos_dist "
                      f"calls), numpy benchmark.py restatement, {dt:.1f} s"}


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-reps", type=int, default=3, help="0: skip the binned_cosine composition")
    ap.add_argument("--cpu-sample", type=int, default=0, help="clusters timed on 1 host core (0: skip)")
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    if args.cpu_only:
        print(json.dumps({"cpu_baseline": cpu_figure(args.cpu_sample or 200)}), flush=True)
        return
    import torch

    from specpride_amd import engine
    from specpride_amd.synthetic import make_clusters_torch

    b = engine.DeviceBatch.from_device(make_clusters_torch(args.clusters, seed=0))
    C, S, P = b.n_clusters, b.n_spectra, b.n_peaks
    res = engine.cosine_medoid(b, with_scores=True)
    for _ in range(args.warmup):
        engine.cosine_medoid(b, out=res)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        engine.cosine_medoid(b, out=res)
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    st = res.status[:C]
    new = spread(ms)
    nbytes = 16 * P + 8 * S
    sizes = torch.as_tensor(np.diff(b.host_cluster_off), device=b.device)
    out = {"workload": "configs[1] batch: the member of every cluster with the highest average binned cosine",
           "clusters": C, "spectra": S, "peaks": P, "pairs": int((sizes * (sizes + 1) // 2).sum().item()),
           "cosine_medoid": new, "clusters_per_s": round(C / (new["median_ms"] * 1e-3), 1),
           "algorithmic_bytes": nbytes, "algorithmic_GBs": round(nbytes / (new["median_ms"] * 1e-3) / 1e9, 1),
           "workspace_bytes": int(b._bufs["cosine_medoid"].numel()),
           "status_ok": int((st == 0).sum().item())}
    if args.baseline_reps > 0:
        co, so = b.t["cluster_off"], b.t["spec_off"]
        max_n = int(sizes.max().item())
        samples = [0.0] * args.baseline_reps
        agree, worst = 0, 0.0
        score_k = torch.empty(C, dtype=torch.float64, device=b.device)
        best = torch.full((C,), -1.0, dtype=torch.float64, device=b.device)
        best_k = torch.zeros(C, dtype=torch.int64, device=b.device)
        cres = None
        for k in range(max_n):
            idx = co[:-1] + torch.clamp(torch.full_like(sizes, k), max=sizes - 1)
            lens = so[idx + 1] - so[idx]
            rep_off = torch.zeros(C + 1, dtype=torch.int64, device=b.device)
            torch.cumsum(lens, 0, out=rep_off[1:])
            src = torch.repeat_interleave(so[idx] - rep_off[:-1], lens) + torch.arange(int(rep_off[-1].item()),
                                                                                        device=b.device)
            rep_mz, rep_int = b.t["mz"][src], b.t["inten"][src]
            mrp = int(lens.max().item())
            cres = engine.binned_cosine(b, rep_off, rep_mz, rep_int, out=cres, max_rep_peaks=mrp)  # warm-up
            torch.cuda.synchronize()
            for r in range(args.baseline_reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                engine.binned_cosine(b, rep_off, rep_mz, rep_int, out=cres, max_rep_peaks=mrp)
                ev[1].record()
                torch.cuda.synchronize()
                samples[r] += ev[0].elapsed_time(ev[1])
            live = sizes > k
            score_k.copy_(cres.avg[:C])
            mine = res.score[:S][idx]
            rel = ((score_k - mine).abs() / mine.abs().clamp(min=1e-300))[live]
            worst = max(worst, float(rel.max().item()) if rel.numel() else 0.0)
            better = live & (score_k > best)
            best = torch.where(better, score_k, best)
            best_k = torch.where(better, torch.full_like(best_k, k), best_k)
        agree = int(((co[:-1] + best_k) == res.rep[:C]).sum().item())
        base = spread(samples)
        out["baseline_binned_cosine_composition"] = dict(base, calls=max_n)
        out["speedup_median"] = round(base["median_ms"] / new["median_ms"], 2)
        out["baseline_check"] = {"max_rel_score_diff": worst, "same_rep": agree, "clusters": C,
                                 "note": "the composition does not tie n = 2 clusters bit for bit"}
    if args.cpu_sample > 0:
        out["cpu_baseline"] = cpu_figure(args.cpu_sample)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
