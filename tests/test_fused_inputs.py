"""The fused pass's edge inputs (tests/fused_cases.py): proof that they are what they claim.

No GPU here.  Every builder's named property is asserted on the host -- the medoid's
column count K through ``np_oracle.xcorr_bins``, the distinct bin-mean bins D through the
bin formula of ``np_oracle.bin_mean_cluster``, the peaks on each side of the range, the
exact lengths, the bins 32,767 and 32,768, the ties -- and the two oracles are shown to
agree on every case (bin-mean bit for bit, medoid representatives equal, totals bit for
bit), which is the anchor tests/test_gpu_fused.py leans on.
"""
import os
import re

import numpy as np
import pytest

import fused_cases as fc
from oracle import c_oracle, np_oracle

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "specpride_amd", "csrc")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _spectrum(csr, c, j):
    return csr.spectrum(csr.cluster_off[c] + j)[0]


def test_constants_match_the_kernel_sources():
    """The table at the top of fused_cases.py against the sources it cites."""
    with open(os.path.join(CSRC, "bin_mean.hip")) as fh:
        bm = fh.read()
    with open(os.path.join(CSRC, "medoid.hip")) as fh:
        md = fh.read()
    assert re.search(r"#define SPX_BR_NMAX (\d+)", bm).group(1) == str(fc.BR_NMAX)
    assert re.search(r"constexpr int BM_FASTLEN = 4 \* 63;", bm) and fc.BM_FASTLEN == 4 * fc.WAVE_PEAKS
    assert re.search(r"constexpr int BM_WMAX = (\d+);", bm).group(1) == str(fc.BM_WMAX)
    assert re.search(r"constexpr int BM_DCAP = (\d+);", bm).group(1) == str(fc.BM_DCAP)
    assert 32 * int(re.search(r"constexpr int BR_MDW32 = (\d+);", bm).group(1)) == fc.MD_BINS
    assert re.search(r"#define SPX_MD_KWMAX (\d+)", md).group(1) == str(fc.MD_KWMAX)


# ------------------------------------------------------------------ the oracles agree
@pytest.mark.parametrize("name", list(fc.CASES))
def test_oracles_agree(name):
    """c_oracle == np_oracle on every case and parameter set: bin-mean bit-exact; medoid
    representatives equal wherever the reference's minimum total is unique, and the C
    totals the very bits of the numpy restatement."""
    csr, _ = fc.case(name)
    for kw, tol in fc.runs(name):
        a, b = c_oracle.bin_mean(csr, **kw), np_oracle.bin_mean(csr, **kw)
        for k in ("status", "out_off", "charge"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
        for k in ("out_mz", "out_int", "prec"):
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{name} {k}")
    for tol in sorted({t for _, t in fc.runs(name)}):
        rep, tot = c_oracle.medoid(csr, tol=tol, with_totals=True)
        for c in range(csr.n_clusters):
            s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
            k, t = np_oracle.medoid_cluster([m for m, _ in csr.cluster(c)], tol)
            np.testing.assert_array_equal(_bits(tot[s0:s1]), _bits(t), err_msg=f"{name} cluster {c} totals")
            if np.count_nonzero(t == t.min()) == 1:
                assert rep[c] == s0 + k, (name, c)
            else:  # a shared minimum: both restate numpy's first argmin
                assert rep[c] == s0 + int(np.flatnonzero(t == t.min())[0]), (name, c)


# ------------------------------------------------------------------ out_of_range
@pytest.mark.parametrize("name", ["out_of_range", "out_of_range_narrow"])
def test_out_of_range_properties(name):
    csr, f = fc.case(name)
    for kw, tol in fc.runs(name):
        p = fc.bin_kw(**kw)
        lo, hi = p["minimum"], p["maximum"]
        assert csr.mz.min() >= 50.0 and csr.mz.max() <= 2600.0
        sizes = np.diff(csr.cluster_off)
        assert sizes.min() >= 2 and sizes.max() <= 12
        lens = np.diff(csr.spec_off)
        assert lens.min() >= 20 and lens.max() <= 125
        # peaks on each side of the range, in the batch and in the edges cluster
        assert np.count_nonzero(csr.mz < lo) >= 50 and np.count_nonzero(csr.mz >= hi) >= 100
        assert np.count_nonzero(fc.in_range(csr.mz, **kw)) >= 1000
        e = f["edges"]
        for j in range(int(sizes[e])):
            mz = _spectrum(csr, e, j)
            assert lo in mz and hi in mz and np.nextafter(hi, 0.0) in mz
            assert np.count_nonzero(mz < lo) >= 1 and np.count_nonzero(mz > hi) >= 1
        # the range's ends: minimum and nextafter(maximum, 0) are in, maximum is out
        np.testing.assert_array_equal(fc.in_range(f["ends"], **kw), [True, True, False])
        # a spectrum wholly out of range, in a cluster that is not
        c, j = f["spectrum_out"]
        mz = _spectrum(csr, c, j)
        assert len(mz) >= 40 and not fc.in_range(mz, **kw).any()
        assert np.any(mz < lo) and np.any(mz >= hi)
        assert fc.cluster_D(csr, c, **kw) > 0
        others = np.concatenate([_spectrum(csr, c, i) for i in range(int(sizes[c])) if i != j])
        assert len(np.intersect1d(np_oracle.xcorr_bins(mz, tol), np_oracle.xcorr_bins(others, tol))) >= 10
        # a cluster wholly out of range: no occupied bin, nothing emitted
        c = f["cluster_out"]
        assert fc.cluster_D(csr, c, **kw) == 0 and len(fc.cluster_mz(csr, c)) >= 100
        ref = c_oracle.bin_mean(csr, **kw)
        assert ref["status"][c] == 0 and ref["out_off"][c + 1] == ref["out_off"][c]
        # every cluster here stays on the register path: the decisions under test are its own
        assert all(fc.fits_register_path(csr, c, tol, **kw) for c in range(csr.n_clusters))


@pytest.mark.parametrize("name", ["out_of_range", "out_of_range_narrow"])
def test_out_of_range_medoid_needs_the_dropped_peaks(name):
    """The flip cluster: the oracle's medoid over the full spectra differs from its medoid
    over the spectra clipped to the bin-mean range, and neither minimum is shared.  A fused
    pass whose medoid followed the bin-mean's range test would return the clipped answer."""
    csr, f = fc.case(name)
    c = f["flip"]
    s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
    for kw, tol in fc.runs(name):
        full, tf = c_oracle.medoid(csr, tol=tol, with_totals=True)
        cut, tc = c_oracle.medoid(fc.clipped(csr, **kw), tol=tol, with_totals=True)
        assert full[c] != cut[c]
        assert cut[c] == s0 and full[c] > s0
        for t in (tf[s0:s1], tc[s0:s1]):
            assert np.count_nonzero(t == t.min()) == 1
        # and it is not the only one: clipping moves totals in the other clusters too
        assert np.count_nonzero(_bits(tf) != _bits(tc)) > s1 - s0


# ------------------------------------------------------------------ lengths
def test_lengths_properties():
    csr, f = fc.case("lengths")
    seen = set()
    for c, lens in f["lengths"].items():
        assert len(lens) in (3, 4)
        np.testing.assert_array_equal(fc.spectrum_lengths(csr, c), lens)
        seen.update(lens)
    assert seen == set(fc.LENGTHS)
    assert max(fc.spectrum_lengths(csr, f["long"])) == fc.BM_FASTLEN + 1
    for c in range(csr.n_clusters):
        assert fc.fits_register_path(csr, c) == (c != f["long"]), c
    short, fs = fc.lengths(with_253=False)
    assert fs["long"] is None and np.diff(short.spec_off).max() == fc.BM_FASTLEN
    assert all(fc.fits_register_path(short, c) for c in range(short.n_clusters))
    # the seams: peaks i, i + 1 straddle two waves (i = 63 w + 62)
    assert fc.SEAMS == tuple(fc.WAVE_PEAKS * (w + 1) - 1 for w in range(3))
    for i in fc.SEAMS:
        for key, same in (("seam_same", True), ("seam_diff", False)):
            c, spectra = f[key][i]
            for j in spectra:
                mz = _spectrum(csr, c, j)
                assert len(mz) >= i + 2
                a, b = mz[i:i + 2]
                assert a < b and fc.in_range([a, b]).all()
                bins = fc.bin_mean_bins([a, b])
                md = np.ceil(np.array([a, b]) / 0.1)
                assert (bins[0] == bins[1]) == same and (md[0] == md[1]) == same, (i, key, j)


# ------------------------------------------------------------------ counts
def test_counts_properties():
    csr, f = fc.case("counts")
    sizes = np.diff(csr.cluster_off)
    for c, n in f["sizes"].items():
        assert sizes[c] == n
    assert sorted(set(f["sizes"].values())) == [1, 2, 3, 49, 50, 51]
    assert sizes[f["over"]] == fc.BR_NMAX + 1
    lens = fc.spectrum_lengths(csr, f["empty_last"])
    assert len(lens) == fc.BR_NMAX and lens[-1] == 0 and lens[:-1].min() > 0
    lens = fc.spectrum_lengths(csr, f["empty_middle"])
    assert len(lens) == 3 and lens[1] == 0 and lens[0] > 0 and lens[2] > 0
    assert 20 <= np.median(np.diff(csr.spec_off)) <= 40
    # odd and even n, a last even spectrum (n odd) among them
    assert {int(n) % 2 for n in sizes} == {0, 1}
    for c in range(csr.n_clusters):
        assert fc.fits_register_path(csr, c) == (c != f["over"]), c
    small, fs = fc.counts(with_51=False)
    assert np.diff(small.cluster_off).max() == fc.BR_NMAX
    assert all(fc.fits_register_path(small, c) for c in range(small.n_clusters))


# ------------------------------------------------------------------ k_columns / d_bins
def test_k_columns_properties():
    csr, f = fc.case("k_columns")
    assert sorted(f["K"].values()) == [64, 65, fc.MD_KMAX, fc.MD_KMAX + 1]
    _, tot = c_oracle.medoid(csr, with_totals=True)
    for c, K in f["K"].items():
        assert fc.cluster_K(csr, c) == K
        assert len(np.unique(np.ceil(fc.cluster_mz(csr, c) / 0.1))) == K
        # the only cap this cluster is near is K's
        assert fc.cluster_D(csr, c) <= 1000 < fc.BM_DCAP
        assert fc.spectrum_lengths(csr, c).max() <= fc.BM_FASTLEN
        assert fc.fits_register_path(csr, c) == (K <= fc.MD_KMAX)
        t = tot[csr.cluster_off[c]:csr.cluster_off[c + 1]]
        assert np.count_nonzero(t == t.min()) == 1 and len(np.unique(t)) > 2
    fit, ff = fc.k_columns(Ks=(64, 65, fc.MD_KMAX))
    assert all(fc.fits_register_path(fit, c) for c in range(fit.n_clusters))
    assert sorted(fc.cluster_K(fit, c) for c in ff["K"]) == [64, 65, fc.MD_KMAX]


def test_d_bins_properties():
    csr, f = fc.case("d_bins")
    assert sorted(f["D"].values()) == [fc.BM_DCAP, fc.BM_DCAP + 1]
    _, tot = c_oracle.medoid(csr, with_totals=True)
    ref = c_oracle.bin_mean(csr)
    for c, D in f["D"].items():
        assert fc.cluster_D(csr, c) == D
        assert fc.in_range(fc.cluster_mz(csr, c)).all()
        assert fc.cluster_K(csr, c) <= fc.MD_KMAX and fc.spectrum_lengths(csr, c).max() <= fc.BM_FASTLEN
        assert fc.fits_register_path(csr, c) == (D <= fc.BM_DCAP)
        assert ref["out_off"][c + 1] - ref["out_off"][c] >= 12  # the common bins pass the quorum
        t = tot[csr.cluster_off[c]:csr.cluster_off[c + 1]]
        assert np.count_nonzero(t == t.min()) == 1
    fit, ff = fc.d_bins(Ds=(fc.BM_DCAP,))
    assert all(fc.fits_register_path(fit, c) for c in range(fit.n_clusters))
    assert [fc.cluster_D(fit, c) for c in ff["D"]] == [fc.BM_DCAP]


# ------------------------------------------------------------------ medoid_range
@pytest.mark.parametrize("tol", [0.1, 0.02])
def test_medoid_range_properties(tol):
    csr, f = fc.case(f"medoid_range_{tol}")
    last, first = fc.MD_BINS - 1, fc.MD_BINS
    assert np.ceil(f["mz_in"] / tol) == last and np.ceil(f["mz_out"] / tol) == first
    # beyond the default bin-mean range at 0.1, inside it at 0.02
    assert bool(fc.in_range([f["mz_in"]])[0]) == (tol == 0.02)
    bins = lambda c: np_oracle.xcorr_bins(fc.cluster_mz(csr, c), tol)  # noqa: E731
    sbins = lambda c, j: np_oracle.xcorr_bins(_spectrum(csr, c, j), tol)  # noqa: E731
    assert bins(f["last_in"]).max() == last and bins(f["last_in"]).min() == 0
    assert 0.0 in fc.cluster_mz(csr, f["last_in"])
    assert fc.fits_register_path(csr, f["last_in"], tol)
    c = f["first_out"]
    assert bins(c).max() == first and bins(c).min() == 0
    assert 0 in sbins(c, 0) and first not in sbins(c, 0)
    assert first in sbins(c, 1) and 0 not in sbins(c, 1)
    c = f["both"]
    lowest = bins(c).min()
    assert {last, first} <= set(bins(c))
    for j in (0, 3):
        assert first in sbins(c, j) and lowest in sbins(c, j)
    for c in range(csr.n_clusters):
        assert fc.fits_register_path(csr, c, tol) == (c not in (f["first_out"], f["both"])), c


# ------------------------------------------------------------------ ceil_ties
def test_ceil_ties_properties():
    csr, f = fc.case("ceil_ties")
    # every m/z is a 5-decimal multiple of 0.05, and multiples of each tolerance are there
    k = np.round(csr.mz / 0.05)
    np.testing.assert_array_equal(csr.mz, np.round(k * 0.05, 5))
    assert np.count_nonzero(k % 2 == 0) > 500 and np.count_nonzero(k % 6 == 0) > 100
    for _, tol in fc.runs("ceil_ties"):
        q = csr.mz / tol
        # the quotient is within the kernels' uncertainty band (2^-24) of an integer
        assert np.count_nonzero(np.abs(q - np.round(q)) < 2.0 ** -24) > 100, tol
        # several peaks per medoid bin within one spectrum (on this 0.05 grid a bin of
        # 0.05 holds one m/z: only the wider tolerances can have it)
        dup = 0
        for s in range(csr.n_spectra):
            mz = csr.spectrum(s)[0]
            dup += len(mz) - len(np_oracle.xcorr_bins(mz, tol))
        assert dup > 50 if tol > 0.05 else dup == 0, tol
        # the ties are ties: the named spectra share the minimal total, bit for bit
        rep, tot = c_oracle.medoid(csr, tol=tol, with_totals=True)
        for c, who in f["ties"].items():
            s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
            t = tot[s0:s1]
            assert tuple(np.flatnonzero(_bits(t) == _bits(t)[np.argmin(t)])) == who, (tol, c)
            assert rep[c] == s0 + who[0]
    # exact m/z ties across spectra
    c = 0
    a, b = _spectrum(csr, c, 0), _spectrum(csr, c, 1)
    assert len(np.intersect1d(a, b)) > 30
    assert all(fc.fits_register_path(csr, c, 0.05) for c in range(csr.n_clusters))


# ------------------------------------------------------------------ wide_params / deferrals
def test_wide_params_properties():
    csr, _ = fc.case("wide_params")
    (kw, tol), = fc.runs("wide_params")
    assert fc.n_words(**kw) > fc.BM_WMAX >= fc.n_words()
    for c in range(csr.n_clusters):  # ordinary under the default parameters, nowhere under these
        assert fc.fits_register_path(csr, c) and not fc.fits_register_path(csr, c, tol, **kw)


def test_deferrals_properties():
    csr, _ = fc.case("deferrals")
    sizes = np.diff(csr.cluster_off)
    assert csr.n_clusters == 40 and sizes.min() >= 2 and sizes.max() <= 23
    assert csr.mz.max() <= 4500.1
    past = [np_oracle.xcorr_bins(fc.cluster_mz(csr, c)).max() >= fc.MD_BINS for c in range(csr.n_clusters)]
    assert sum(past) >= 30  # deferred at run time: nothing about their size says so
    assert np.diff(csr.spec_off).max() <= fc.BM_FASTLEN
