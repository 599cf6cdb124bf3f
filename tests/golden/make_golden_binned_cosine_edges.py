#!/usr/bin/env python3
"""Generate tests/golden/binned_cosine_edges.npz by running the REFERENCE's own
``benchmark.cos_dist`` / ``average_cos_dist`` (src/benchmark.py:19-38) on the named
cases of ``tests/binned_cosine_cases.py``; the ``mz_space_*`` cases run with
``benchmark.mz_space`` set to their spacing.  Runs only where the reference checkout
exists (the path and the import stand-ins are make_golden.py's).

Stored: every case's clusters one after the other as one CSR batch with their
representatives (``rep_off`` / ``rep_mz`` / ``rep_int``), ``cos`` [S], ``avg`` [C],
``status`` [C], and per case its name, first cluster (``case_off``) and ``mz_space``.
"""
from __future__ import annotations

import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_SRC, REPO, STATUS_EMPTY, STATUS_OK, STUBS, _csr_arrays  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
import binned_cosine_cases as cases  # noqa: E402
from specpride_amd.csr import SpectraCSR  # noqa: E402


def main():
    sys.path.insert(0, STUBS)
    sys.path.insert(0, REF_SRC)
    bench = importlib.import_module("benchmark")
    default_space = bench.mz_space
    assert default_space == cases.MZ_SPACE
    names = list(cases.CASES)
    clusters, reps, case_off, spaces = [], [], [0], []
    cos, avg, status = [], [], []
    for name in names:
        bench.mz_space = cases.mz_space_of(name)
        for spectra, (rm, ri) in cases.clusters_of(name):
            rep = SimpleNamespace(mz=rm, intensity=ri)
            members = [SimpleNamespace(mz=m, intensity=i) for m, i in spectra]
            try:
                with np.errstate(invalid="ignore", over="ignore"):
                    cs = [bench.cos_dist(rep, mem) for mem in members]
                    avg.append(bench.average_cos_dist(rep, members))
                cos.extend(cs)
                status.append(STATUS_OK)
            except IndexError:  # mz[-1] of an empty spectrum (benchmark.py:20)
                cos.extend([np.nan] * len(spectra))
                avg.append(np.nan)
                status.append(STATUS_EMPTY)
            clusters.append(spectra)
            reps.append((rm, ri))
        case_off.append(len(clusters))
        spaces.append(bench.mz_space)
        print(f"{name}: {case_off[-1] - case_off[-2]} clusters", flush=True)
    bench.mz_space = default_space
    csr = SpectraCSR.from_clusters([[{"m/z array": m, "intensity array": i} for m, i in sp] for sp in clusters])
    rep_off = np.zeros(len(reps) + 1, np.int64)
    np.cumsum([len(r[0]) for r in reps], out=rep_off[1:])
    np.savez_compressed(os.path.join(HERE, "binned_cosine_edges.npz"), **_csr_arrays(csr),
                        rep_off=rep_off, rep_mz=np.concatenate([r[0] for r in reps]),
                        rep_int=np.concatenate([r[1] for r in reps]),
                        cos=np.array(cos, np.float64), avg=np.array(avg, np.float64), status=np.array(status, np.int32),
                        case_names=np.array(names), case_off=np.array(case_off, np.int64),
                        case_mz_space=np.array(spaces, np.float64))
    print(f"binned_cosine_edges: {len(names)} cases, {len(clusters)} clusters, {len(cos)} members")


if __name__ == "__main__":
    main()
