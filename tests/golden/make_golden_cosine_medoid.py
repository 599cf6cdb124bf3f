#!/usr/bin/env python3
"""Generate tests/golden/cosine_medoid.npz by running the REFERENCE's own
``benchmark.average_cos_dist`` (src/benchmark.py:31-38) with every member of a cluster
as the representative in turn, on the clusters of ``tests/cosine_medoid_cases.py``
(``golden_clusters``).  Runs only where the reference checkout exists (the path and
the import stand-ins are make_golden.py's).

Stored: the inputs (CSR arrays), ``score`` [S] = average_cos_dist(member, members) and
``rep`` [C] = the global index of the first member with the maximal score.
"""
from __future__ import annotations

import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_SRC, REPO, STUBS, _csr_arrays  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
import cosine_medoid_cases as cases  # noqa: E402


def main():
    sys.path.insert(0, STUBS)
    sys.path.insert(0, REF_SRC)
    bench = importlib.import_module("benchmark")
    clusters = cases.golden_clusters()
    score, rep, first = [], [], 0
    for members in clusters:
        objs = [SimpleNamespace(mz=m, intensity=i) for m, i in members]
        sc = [bench.average_cos_dist(o, objs) for o in objs]
        best = 0
        for i in range(1, len(sc)):
            if sc[i] > sc[best]:
                best = i
        score.extend(sc)
        rep.append(first + best)
        first += len(members)
    csr = cases.to_csr(clusters)
    np.savez_compressed(os.path.join(HERE, "cosine_medoid.npz"), **_csr_arrays(csr),
                        mz_space=np.float64(bench.mz_space), score=np.array(score, np.float64),
                        rep=np.array(rep, np.int64))
    print(f"cosine_medoid: {len(clusters)} clusters, {len(score)} members")


if __name__ == "__main__":
    main()
