"""The four workspace size queries return what they returned before the host API's layouts
were folded into one carve_* function per method (csrc/spx_api.hip): every size is pinned
in golden/workspace_sizes.json.  The queries are pure host functions -- they read the scalar
fields of spx_csr and, for medoid, two host offset arrays -- so they run without a GPU.

The golden file is recorded from a build of the commit whose sizes are to be kept:
    SPX_LIB=/path/to/that/libspecpride_hip.so python tests/test_workspace_layout.py
"""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from specpride_amd import _lib  # noqa: E402

GOLDEN_FILE = os.path.join(REPO, "tests", "golden", "workspace_sizes.json")

# Thresholds of the layouts, copied from csrc/*.hip (the library does not export them).  If one
# changes there, the pinned sizes change and this test fails; update the copy here with the golden
# file then, or the each-side-of-the-threshold cases below no longer straddle the boundary.
GA_GIANT_N, GA_OWN_N = 16384, 65536
BM_NMAX = 128
MD_NMAX, MW_PMAX, MW_KWMAX = 64, 32768, 95
CS_RCAP = 512


def _bind(path):
    L = ctypes.CDLL(path)
    p, i64, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
    for name, args in (("spx_bin_mean_workspace_size", [p, p, p]), ("spx_gap_average_workspace_size", [p, p, p]),
                       ("spx_medoid_workspace_size", [p, p, i64, p, i64]),
                       ("spx_binned_cosine_workspace_size", [i64, i64])):
        getattr(L, name).restype = sz
        getattr(L, name).argtypes = args
    return L


def _csr(C, S, P):
    return _lib.SpxCsr(C, S, P, None, None, None, None, None, None, None)


def _offsets(clusters):
    """Host cluster and spectrum offsets of clusters given as (spectra, peaks) pairs."""
    hco, hso = [0], [0]
    for n, p in clusters:
        hco.append(hco[-1] + n)
        for k in range(n):  # the peaks spread over the spectra, the remainder on the first
            hso.append(hso[-1] + p // n + (p % n if k == 0 else 0))
    return np.asarray(hco, np.int64), np.asarray(hso, np.int64)


def workspace_sizes(L, setenv):
    """Every case's name -> size.  ``setenv(name, value or None)`` sets or clears an
    environment variable the library reads."""
    out = {}
    ref = ctypes.byref
    for acc in (0.01, 0.5):
        prm = _lib.SpxGapParams(acc, 1000.0, 0.5, 1.00727646688, 0, 0)
        for C in (0, 1, 1000):
            csr = _csr(C, 10 * C, 200000 * C)
            for maxp in (GA_GIANT_N, GA_GIANT_N + 1, GA_OWN_N, GA_OWN_N + 1):
                for span in (0.0, 1500.0, float("inf"), float("nan")):
                    info = _lib.SpxBatchInfo(maxp, 240, span)
                    out[f"gap acc={acc} C={C} maxp={maxp} span={span}"] = \
                        L.spx_gap_average_workspace_size(ref(csr), ref(prm), ref(info))
    for seg in (None, "0"):
        setenv("SPX_SEG_ARENA", seg)
        for cap in (None, "4"):
            setenv("SPX_SPLIT_RANGE_CAP", cap)
            for binsize in (0.02, 0.0001):
                prm = _lib.SpxBinParams(100.0, 2000.0, binsize, 1)
                for C in (0, 1000):
                    csr = _csr(C, 20 * C, 2000 * C)
                    for maxs in (BM_NMAX, BM_NMAX + 1):
                        info = _lib.SpxBatchInfo(5000, maxs, 1500.0)
                        out[f"bin_mean seg_arena={seg} range_cap={cap} binsize={binsize} C={C} maxs={maxs}"] = \
                            L.spx_bin_mean_workspace_size(ref(csr), ref(prm), ref(info))
    setenv("SPX_SEG_ARENA", None)
    setenv("SPX_SPLIT_RANGE_CAP", None)
    small = [(5, 50)] * 10
    medoid = {
        "C=0": ([], []),
        "small": (small, []),
        "n=MD_NMAX": (small + [(MD_NMAX, 640)], []),
        "n=MD_NMAX+1": (small + [(MD_NMAX + 1, 650)], []),
        "p=MW_PMAX": (small + [(8, MW_PMAX)], []),
        "p=MW_PMAX+1": (small + [(8, MW_PMAX + 1)], []),
        # more than 256 clusters at risk of a run-time deferral: the 256 largest are reserved
        "at_risk=300": ([(4, 64 * MW_KWMAX + 1 + 37 * k) for k in range(300)], []),
        "extra": (small, [1, 3]),
        "extra out of range": (small, [10]),
    }
    for name, (clusters, extra) in medoid.items():
        hco, hso = _offsets(clusters)
        ex = np.asarray(extra, np.int64)
        out[f"medoid {name}"] = L.spx_medoid_workspace_size(hco.ctypes.data, hso.ctypes.data, len(clusters),
                                                            ex.ctypes.data if len(ex) else None, len(ex))
    for C in (0, 1, 1000):
        for maxr in (0, CS_RCAP, CS_RCAP + 1, 100000):
            out[f"cosine C={C} maxr={maxr}"] = L.spx_binned_cosine_workspace_size(C, maxr)
    out["cosine C=-1 maxr=5"] = L.spx_binned_cosine_workspace_size(-1, 5)
    out["cosine C=5 maxr=-1"] = L.spx_binned_cosine_workspace_size(5, -1)
    return out


def test_workspace_sizes_are_pinned(monkeypatch):
    def setenv(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)

    with open(GOLDEN_FILE) as fh:
        want = json.load(fh)
    got = workspace_sizes(_bind(_lib.build()), setenv)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    # the invalid queries say so, every other one asks for room
    zero = sorted(k for k, v in want.items() if v == 0)
    assert zero == ["cosine C=-1 maxr=5", "cosine C=5 maxr=-1", "medoid extra out of range"]


if __name__ == "__main__":
    def _setenv(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value

    sizes = workspace_sizes(_bind(_lib.LIB_PATH), _setenv)  # (no build: SPX_LIB names the library to record)
    with open(GOLDEN_FILE, "w") as fh:
        json.dump(sizes, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(sizes)} sizes from {_lib.LIB_PATH} -> {GOLDEN_FILE}")
