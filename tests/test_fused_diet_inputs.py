"""The inputs of tests/fused_diet_cases.py: proof that they are what they claim.

No GPU here.  The band classes are checked with the kernel's arithmetic restated in numpy
float64 (IEEE, never fused), the bins with the oracle's own formulas, and the two oracles
are shown to agree on every batch, which is what tests/test_gpu_fused_diet.py leans on.
"""
import numpy as np
import pytest

import fused_cases as fc
import fused_diet_cases as dc
from oracle import c_oracle, np_oracle

BATCHES = ("band_edges", "idle_lanes", "seams", "packing", "sequence")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _spectrum(csr, c, j):
    return csr.spectrum(csr.cluster_off[c] + j)[0]


def _md_bins(mz, tol=dc.TOL):
    return np.ceil(np.asarray(mz, np.float64) / tol).astype(np.int64)


@pytest.mark.parametrize("name", BATCHES)
def test_batches_are_small_and_the_oracles_agree(name):
    csr, _ = dc.case(name)
    assert csr.n_clusters <= 8
    for kw in (dict(), dc.NO_QUORUM):
        a, b = c_oracle.bin_mean(csr, **kw), np_oracle.bin_mean(csr, **kw)
        for k in ("status", "out_off", "charge"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
        for k in ("out_mz", "out_int", "prec"):
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{name} {k}")
    rep, tot = c_oracle.medoid(csr, tol=dc.TOL, with_totals=True)
    for c in range(csr.n_clusters):
        s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
        _, t = np_oracle.medoid_cluster([m for m, _ in csr.cluster(c)], dc.TOL)
        np.testing.assert_array_equal(_bits(tot[s0:s1]), _bits(t), err_msg=f"{name} cluster {c} totals")
        assert rep[c] == s0 + int(np.flatnonzero(t == t.min())[0]), (name, c)


# ------------------------------------------------------------------ band_edges
@pytest.mark.parametrize("which", ["bm", "md"])
def test_band_classes_are_all_populated(which):
    """Every class of fraction holds an m/z, for the bin-mean's bins and for the medoid's:
    exactly 0, inside the band on either side, the last fraction inside and the first
    outside on either side.  So the division path (five classes) and the fast path next to
    it (two) each decide bins; and the m/z are in the cluster, on owner lanes, in range."""
    csr, f = dc.case("band_edges")
    fraction, band = (dc.bm_fraction, dc.BM_BAND) if which == "bm" else (dc.md_fraction, dc.MD_BAND)
    holders = [_spectrum(csr, f["cluster"], 0)] + ([_spectrum(csr, f["cluster"], 1)] if which == "bm" else [])
    for cls in dc.CLASSES:
        mzs = np.array(f[which][cls])
        assert len(mzs) >= 1, (which, cls)
        q, fr = fraction(mzs)
        assert np.all(dc.classify(q, fr, band) == cls)
        # the kernel's predicate: the fast path where b < f < 1 - b, else the division
        fast = (fr > band) & (fr < 1.0 - band)
        assert np.all(fast == (cls in dc.FAST_CLASSES)), (which, cls)
        assert np.all(fc.in_range(mzs))
        for h in holders:
            assert np.all(np.isin(mzs, h))
    lens = fc.spectrum_lengths(csr, f["cluster"])
    assert lens.max() <= fc.BM_FASTLEN and fc.fits_register_path(csr, f["cluster"])


def test_band_fast_path_answers_are_the_divisions():
    """On the fast classes, the ones right next to the band, the reciprocal product's
    integer part is the oracle's bin: the premise of the band."""
    _, f = dc.case("band_edges")
    for cls in dc.FAST_CLASSES:
        m = np.array(f["bm"][cls])
        q, _ = dc.bm_fraction(m)
        np.testing.assert_array_equal(np.trunc(q).astype(np.int64), fc.bin_mean_bins(m))
        m = np.array(f["md"][cls])
        q, _ = dc.md_fraction(m)
        np.testing.assert_array_equal(np.ceil(q).astype(np.int64), _md_bins(m))


def test_band_neighbours_make_a_wrong_side_visible():
    """The bins on both sides of every special m/z are occupied by another spectrum."""
    csr, f = dc.case("band_edges")
    c = f["cluster"]
    for cls in dc.CLASSES:
        for m in f["bm"][cls]:
            b = int(fc.bin_mean_bins([m])[0])
            for s in (2, 3):
                other = fc.bin_mean_bins(_spectrum(csr, c, s))
                assert np.any(np.abs(other - b) <= 1), (cls, m)
        for m in f["md"][cls]:
            b = int(_md_bins([m])[0])
            assert any(np.any(np.abs(_md_bins(_spectrum(csr, c, s)) - b) <= 1) for s in (1, 2)), (cls, m)


# ------------------------------------------------------------------ idle_lanes
def test_idle_lanes_properties():
    csr, f = dc.case("idle_lanes")
    c = f["lengths"]
    lens = list(fc.spectrum_lengths(csr, c))
    assert lens[:len(dc.IDLE_LENGTHS)] == list(dc.IDLE_LENGTHS) and lens[-1] == 40
    assert len(lens) <= fc.BR_NMAX and fc.fits_register_path(csr, c)
    one = _spectrum(csr, c, f["one_bin"])
    assert len(np.unique(fc.bin_mean_bins(one))) == 1 and len(np.unique(_md_bins(one))) == 1
    assert len(np.unique(one)) == 40 and np.all(fc.in_range(one))
    out = fc.cluster_mz(csr, f["all_out"])
    assert len(out) > 0 and not np.any(fc.in_range(out)) and fc.cluster_D(csr, f["all_out"]) == 0
    assert np.any(out < 100.0) and np.any(out >= 2000.0)


# ------------------------------------------------------------------ seams
def test_seam_properties():
    csr, f = dc.case("seams")
    for c, same in ((f["same"], True), (f["diff"], False)):
        assert list(fc.spectrum_lengths(csr, c)) == [252, 252, 252]
        for s in range(3):
            mz = _spectrum(csr, c, s)
            assert np.all(fc.in_range(mz))
            b, k = fc.bin_mean_bins(mz), _md_bins(mz)
            for i in fc.SEAMS:
                assert (b[i] == b[i + 1]) == same and (k[i] == k[i + 1]) == same, (c, s, i)
            if not same:
                assert np.all(np.diff(b) > 0)
        assert fc.fits_register_path(csr, c)


# ------------------------------------------------------------------ packing
def test_packing_properties():
    csr, f = dc.case("packing")
    assert sorted(f["sizes"].values()) == sorted(dc.PACK_SIZES)
    for c, n in f["sizes"].items():
        assert csr.cluster_off[c + 1] - csr.cluster_off[c] == n
        assert fc.fits_register_path(csr, c)
        D, K = fc.cluster_D(csr, c), fc.cluster_K(csr, c)
        if n >= 49:  # slots up to 1,529 of BM_DCAP = 1,536; columns up to 1,719 of 1,728
            assert D == 1530 and K == 1720
            assert fc.BM_DCAP - 8 < D <= fc.BM_DCAP and fc.MD_KMAX - 10 < K <= fc.MD_KMAX
        else:        # all that n spectra of BM_FASTLEN peaks can hold
            assert D == K == fc.BM_FASTLEN * n
            assert list(fc.spectrum_lengths(csr, c)) == [fc.BM_FASTLEN] * n


# ------------------------------------------------------------------ sequence
def test_sequence_properties():
    csr, f = dc.case("sequence")
    kinds = f["kinds"]
    assert set(kinds.values()) >= {"full49", "not_here", "band", "mixed_charge", "idle", "all_out", "seam", "full3"}
    by = {k: c for c, k in kinds.items()}
    assert csr.cluster_off[by["not_here"] + 1] - csr.cluster_off[by["not_here"]] == fc.BR_NMAX + 1
    s0, s1 = csr.cluster_off[by["mixed_charge"]], csr.cluster_off[by["mixed_charge"] + 1]
    assert len(np.unique(csr.charge[s0:s1])) == 2
    st = c_oracle.bin_mean(csr)["status"]
    assert st[by["mixed_charge"]] == 1 and np.all(np.delete(st, by["mixed_charge"]) == 0)
    # each early exit is followed by a cluster that runs every phase
    for name in ("not_here", "mixed_charge"):
        assert fc.fits_register_path(csr, by[name] + 1)
