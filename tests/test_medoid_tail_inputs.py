"""Every case of tests/medoid_tail_cases.py HAS the property it is named for: proved on the
host against the oracle, so tests/test_gpu_medoid_tail.py exercises what it says it does."""
import numpy as np
import pytest

import fused_cases as fc
import medoid_tail_cases as tc
from oracle import c_oracle, np_oracle


def _cluster_totals(csr, tot, c):
    return tot[csr.cluster_off[c]:csr.cluster_off[c + 1]]


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_register_path_membership(name):
    """The fused register bodies complete every cluster of a `clean` case, and hand at least
    one on in the others; spectra are tiny except in the row-word cases."""
    csr, facts, clean = tc.case(name)
    fits = [fc.fits_register_path(csr, c, tc.TOL) for c in range(csr.n_clusters)]
    assert all(fits) if clean else not all(fits)
    if not name.startswith("row_words"):
        assert np.diff(csr.spec_off).max() <= 13


def test_sizes_cover_the_edges():
    csr, facts, _ = tc.case("sizes")
    assert tuple(np.diff(csr.cluster_off)) == tc.FUSED_SIZES
    for n in (2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 39, 40, 41, 47, 48, 49, 50, tc.NMIN, tc.NMIN + 1):
        assert n in tc.FUSED_SIZES
    over, _, _ = tc.case("sizes_over")
    assert tuple(np.diff(over.cluster_off)) == (51, 63, 64, 65)


def test_row_words():
    csr, facts, _ = tc.case("row_words")
    kws = set()
    for c, K in facts["K"].items():
        assert fc.cluster_K(csr, c, tc.TOL) == K
        kws.add(((K + 63) // 64) | 1)
    assert {1, 3, fc.MD_KWMAX} <= kws
    over, ofacts, _ = tc.case("row_words_over")
    for c, K in ofacts["K"].items():
        assert fc.cluster_K(over, c, tc.TOL) == K and (((K + 63) // 64) | 1) > fc.MD_KWMAX


def test_empty_spectra_give_distance_one():
    csr, facts, _ = tc.case("empties")
    lens = np.diff(csr.spec_off)
    for c, where in facts["empty"].items():
        s0, n = csr.cluster_off[c], csr.cluster_off[c + 1] - csr.cluster_off[c]
        assert [j for j in range(n) if lens[s0 + j] == 0] == sorted(where)
    _, tot = c_oracle.medoid(csr, tol=tc.TOL, with_totals=True)
    for c, where in facts["empty"].items():
        n = csr.cluster_off[c + 1] - csr.cluster_off[c]
        for j in where:  # d = 1.0 to every spectrum, itself (twice: row and column) included
            assert _cluster_totals(csr, tot, c)[j] == (n + 1) / n


def test_identical_spectra():
    csr, facts, _ = tc.case("identical")
    rep, tot = c_oracle.medoid(csr, tol=tc.TOL, with_totals=True)
    for c in range(csr.n_clusters):
        t = _cluster_totals(csr, tot, c)
        assert np.all(t == t[0]) and rep[c] == csr.cluster_off[c]


def test_two_minima():
    csr, f, _ = tc.case("two_minima")
    rep, tot = c_oracle.medoid(csr, tol=tc.TOL, with_totals=True)
    t = _cluster_totals(csr, tot, f["cluster"])
    assert list(np.flatnonzero(t == t.min())) == [f["lo"], f["hi"]] == [5, 40]
    assert rep[f["cluster"]] == csr.cluster_off[f["cluster"]] + 5


def test_shared_bin_diagonal():
    csr, _, _ = tc.case("shared_bin")
    for s in range(csr.n_spectra):
        mz = csr.mz[csr.spec_off[s]:csr.spec_off[s + 1]]
        assert len(np_oracle.xcorr_bins(mz, tc.TOL)) == len(mz) - 1  # d(i, i) = 1 - (p - 1)/p > 0
