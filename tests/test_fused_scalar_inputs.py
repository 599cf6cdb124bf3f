"""The inputs of tests/fused_scalar_cases.py: proof that they are what they claim.

No GPU here.  Lengths, sizes and positions are read back from the batches, the statuses
come from the C oracle (which the numpy oracle confirms), and the band classes are checked
with the kernel's arithmetic restated in numpy float64, as tests/test_fused_diet_inputs.py
does.  tests/test_gpu_fused_scalar.py leans on all of it.
"""
import numpy as np
import pytest

import fused_cases as fc
import fused_diet_cases as dc
import fused_scalar_cases as sc
import fused_sequences as fs
from oracle import c_oracle, np_oracle

OK, MIXED = 0, 1


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _n(csr, c):
    return int(csr.cluster_off[c + 1] - csr.cluster_off[c])


def _oracles_agree(csr, kw=None, tol=sc.TOL):
    kw = kw or {}
    a, b = c_oracle.bin_mean(csr, **kw), np_oracle.bin_mean(csr, **kw)
    for k in ("status", "out_off", "charge"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in ("out_mz", "out_int"):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
    rep, tot = c_oracle.medoid(csr, tol=tol, with_totals=True)
    for c in range(csr.n_clusters):
        s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
        _, t = np_oracle.medoid_cluster([m for m, _ in csr.cluster(c)], tol)
        np.testing.assert_array_equal(_bits(tot[s0:s1]), _bits(t), err_msg=f"cluster {c} totals")
        assert rep[c] == s0 + int(np.flatnonzero(t == t.min())[0]), c
    return a["status"]


# ------------------------------------------------------------------ mask_edges
def test_mask_edges_properties():
    csr, f = sc.case("mask_edges")
    assert csr.n_clusters <= 300
    # every wave boundary of 63 owned lanes, one below and one above
    assert set(sc.EDGE_LENGTHS) >= {63 * w + d for w in (1, 2, 3) for d in (-1, 0, 1)} | {1, 252}
    for L, c in f["alone"].items():
        assert list(fc.spectrum_lengths(csr, c)) == [L, L]
        assert fc.fits_register_path(csr, c)
    assert sorted(fc.spectrum_lengths(csr, f["mixed"])) == sorted(sc.EDGE_LENGTHS)
    assert fc.fits_register_path(csr, f["mixed"])
    for name, at in (("first", 0), ("middle", 1), ("last", 2)):
        lens = list(fc.spectrum_lengths(csr, f["empty"][name]))
        assert lens[at] == 0 and all(x > 0 for i, x in enumerate(lens) if i != at)
        assert fc.fits_register_path(csr, f["empty"][name])
    assert np.all(_oracles_agree(csr) == OK)


# ------------------------------------------------------------------ ring_depths
def test_ring_depths_properties():
    csr, f = sc.case("ring_depths")
    assert sorted(f["sizes"].values()) == sorted(sc.RING_SIZES)
    assert {sc.PFA - 1, sc.PFA, sc.PFA + 1, 2 * sc.PFA, 2 * sc.PFA + 1, fc.BR_NMAX, fc.BR_NMAX + 1} <= set(sc.RING_SIZES)
    for c, n in f["sizes"].items():
        assert _n(csr, c) == n
        assert fc.fits_register_path(csr, c) == (n <= fc.BR_NMAX)
    lens = fc.spectrum_lengths(csr, f["long"])
    assert lens.max() == fc.BM_FASTLEN + 1 and not fc.fits_register_path(csr, f["long"])
    assert fc.fits_register_path(csr, f["long"] + 1)  # a normal cluster follows
    assert np.all(_oracles_agree(csr) == OK)


# ------------------------------------------------------------------ early_returns
@pytest.mark.parametrize("kind", sc.EARLY_KINDS)
def test_early_returns_properties(kind):
    csr, f = sc.case("early_returns", kind)
    assert csr.n_clusters == 5 and f["at"] == (0, 2, 4)
    st = _oracles_agree(csr)
    for c in f["between"]:
        assert fc.fits_register_path(csr, c) and st[c] == OK
    for c in f["at"]:
        mz = fc.cluster_mz(csr, c)
        s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
        if kind == "mixed_charge":
            assert len(np.unique(csr.charge[s0:s1])) == 2 and st[c] == MIXED
            continue
        assert st[c] == OK
        if kind == "inversion":
            unsorted = [bool(np.any(np.diff(m) < 0)) for m, _ in csr.cluster(c)]
            assert sum(unsorted) == 1
        elif kind == "nan_mz":
            assert np.isnan(mz).sum() == 1
        elif kind == "d_over":
            assert fc.cluster_D(csr, c) == fc.BM_DCAP + 1
        elif kind == "md_out":
            bins = np.ceil(mz / sc.TOL)
            assert bins.max() == fc.MD_BINS and fc.cluster_D(csr, c) <= fc.BM_DCAP
            assert not fc.fits_register_path(csr, c)
        elif kind == "n1":
            assert _n(csr, c) == 1


# ------------------------------------------------------------------ walks
def test_walk_properties():
    csr, _ = sc.case("walk")
    assert csr.n_clusters == 40
    sizes = {_n(csr, c) for c in range(csr.n_clusters)}
    assert min(sizes) < sc.PFA < max(sizes)
    assert all(fc.fits_register_path(csr, c) for c in range(csr.n_clusters))
    assert np.all(_oracles_agree(csr) == OK)
    csr, f = sc.case("walk_ends_off_path")
    assert f["last"] == csr.n_clusters - 1 and not fc.fits_register_path(csr, f["last"])
    assert all(fc.fits_register_path(csr, c) for c in range(f["last"]))
    assert np.all(_oracles_agree(csr) == OK)
    for C in (0, 1, 2):
        assert sc.case("few", C)[0].n_clusters == C


# ------------------------------------------------------------------ band_constants
def test_band_constants_properties():
    csr, f = sc.case("band_constants")
    c = f["cluster"]
    assert csr.n_clusters == 3 and _n(csr, c) == 4
    held = [csr.spectrum(csr.cluster_off[c] + s)[0] for s in (0, 1)]
    for name, p in (("A", sc.PARAMS_A), ("B", sc.PARAMS_B)):
        below, lo, last, hi = f["ends"][name]
        assert below < lo == p["minimum"] and last < hi == p["maximum"]
        assert list(fc.in_range([below, lo, last, hi], **p)) == [False, True, True, False]
        edges = np.array(f["edges"][name])
        assert len(edges) >= 3
        q, fr = dc.bm_fraction(edges, p["minimum"], p["binsize"])
        assert not np.any((fr > dc.BM_BAND) & (fr < 1.0 - dc.BM_BAND))  # the kernel's predicate: they divide
        assert np.all(fc.in_range(edges, **p))
        for h in held:
            assert np.all(np.isin(f["ends"][name], h)) and np.all(np.isin(edges, h))
        # the bin space of both sets fits the register path
        assert fc.n_words(**p) <= fc.BM_WMAX
    assert fc.spectrum_lengths(csr, c).max() <= fc.BM_FASTLEN
    for kw in (sc.PARAMS_A, sc.PARAMS_B):
        assert fc.cluster_D(csr, c, **kw) <= fc.BM_DCAP
        for tol in (sc.TOL_A, sc.TOL_B):
            assert fc.fits_register_path(csr, c, tol, **kw)
            for q in (True, False):
                assert np.all(_oracles_agree(csr, dict(kw, apply_peak_quorum=q), tol) == OK)
    # the two sets give different results: a constant kept from the other call would show
    a, b = c_oracle.bin_mean(csr, **sc.PARAMS_A), c_oracle.bin_mean(csr, **sc.PARAMS_B)
    assert a["out_off"][-1] != b["out_off"][-1]
    ta = c_oracle.medoid(csr, tol=sc.TOL_A, with_totals=True)[1]
    tb = c_oracle.medoid(csr, tol=sc.TOL_B, with_totals=True)[1]
    assert not np.array_equal(ta, tb)
