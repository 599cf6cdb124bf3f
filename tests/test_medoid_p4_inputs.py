"""Every case of tests/medoid_p4_cases.py HAS the property it is named for, proved on the host
against the oracle, and the two-wave hand-off model (tests/medoid_p4_model.py) gives numpy's
sums bit for bit: so tests/test_gpu_medoid_p4.py exercises what it says it does."""
import numpy as np
import pytest

import fused_cases as fc
import medoid_p4_cases as pc
import medoid_p4_model as pm
import medoid_tail_model as tm
from oracle import c_oracle, np_oracle
from test_medoid_tail_model import _bits, _random_d, _tied_d


def _cluster_totals(csr, tot, c):
    return tot[csr.cluster_off[c]:csr.cluster_off[c + 1]]


def _kw(K):
    return ((K + 63) // 64) | 1


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("maker", [_random_d, _tied_d], ids=["random", "ties"])
def test_handoff_model_equals_numpy_bit_for_bit(maker):
    """n = 33..64, every column: the sums two waves form through the hand-off equal
    np.add.reduce on the reference's upper-triangular matrix, and the one-wave walk."""
    rng = np.random.default_rng(12)
    for n in range(33, 65):
        d = maker(n, rng)
        ref = tm.reference_sums(d)
        for j in range(n):
            row, col = pm.handoff_sums(d, j)
            assert _bits(row) == _bits(ref[j][0]), (n, j, "row")
            assert _bits(col) == _bits(ref[j][1]), (n, j, "col")
            assert (row, col) == pm.chain_sums(d, j) == tm.column_sums(d, j)
        t = pm.handoff_totals(d)
        want = tm.reference_totals(d)
        assert np.array_equal(_bits(t), _bits(want)), n
        assert tm.argmin_waves(t) == int(np.flatnonzero(want == want.min())[0]), n


def test_what_crosses_is_enough():
    """The accumulators that do NOT cross would have received +0.0 only: for column tile 0
    row tile 1 adds nothing to a column sum, for column tile 1 row tile 0 nothing to a row sum."""
    for n in (33, 40, 41, 50, 57, 64):
        lim = n - n % 8
        for j in range(n):
            ct = j // 32
            cross = pm.crossing(ct)
            rows_t0, rows_t1 = range(0, 32), range(32, lim)
            if not cross["col_acc"]:  # ct = 0: the column sum is complete after row tile 0
                assert cross["col_sum"] and not any(r <= j for r in rows_t1) and not any(r <= j for r in range(lim, n))
            if not cross["row_acc"]:  # ct = 1: the row sums start at +0.0
                assert not any(r >= j for r in rows_t0)


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_register_path_membership(name):
    csr, facts, fused, clean = pc.case(name)
    fits = [fc.fits_register_path(csr, c, pc.TOL) for c in range(csr.n_clusters)]
    assert all(fits) if clean else not all(fits)
    assert np.diff(csr.cluster_off).max() <= 64
    if not name.startswith("handoff") and name != "diagonal" and name != "stale_handoff":
        assert np.diff(csr.spec_off).max() <= 13


@pytest.mark.parametrize("kw", sorted(pc.ROW_WORDS))
def test_handoff_sizes_and_row_words(kw):
    for name, sizes in ((f"handoff_kw{kw}", pc.FUSED_SIZES), (f"handoff_over_kw{kw}", pc.OVER_SIZES)):
        csr, facts, fused, _ = pc.case(name)
        assert tuple(np.diff(csr.cluster_off)) == sizes and fused == (max(sizes) <= fc.BR_NMAX)
        for c in range(csr.n_clusters):
            K = fc.cluster_K(csr, c, pc.TOL)
            assert K == pc.ROW_WORDS[kw] and _kw(K) == kw
    assert pc.FUSED_SIZES == (33, 39, 40, 41, 47, 48, 49, 50) and pc.OVER_SIZES == (56, 57, 63, 64)
    assert 65 <= pc.ROW_WORDS[3] <= 192 and pc.ROW_WORDS[27] == 1728 and pc.ROW_WORDS[1] == 40
    # what row tile 1 holds at each size: strided groups, tail rows
    kinds = {n: ((n - n % 8 - 32) // 8, n % 8) for n in pc.FUSED_SIZES + pc.OVER_SIZES}
    assert kinds[33] == (0, 1) and kinds[39] == (0, 7)            # only the sequential tail
    assert kinds[40] == (1, 0) and kinds[48] == (2, 0) and kinds[56] == (3, 0) and kinds[64] == (4, 0)  # no tail
    assert kinds[41] == (1, 1) and kinds[49] == (2, 1) and kinds[57] == (3, 1)  # groups and a tail


def test_reordered_sums_expose_the_order():
    csr, facts, _, _ = pc.case("reordered")
    assert sorted(facts["n"].values()) == [41, 50]
    _, tot = c_oracle.medoid(csr, tol=pc.TOL, with_totals=True)
    for c, n in facts["n"].items():
        d = pc.distances(csr, c)
        assert d.shape == (n, n) and facts["columns"][c]
        right = pm.handoff_totals(d)
        wrong = pm.handoff_totals(d, tile_order=(1, 0))
        assert np.array_equal(_bits(right), _bits(_cluster_totals(csr, tot, c)))  # the oracle's bits
        changed = [j for j in range(n) if _bits(right[j]) != _bits(wrong[j])]
        assert changed and set(changed) >= set(facts["columns"][c])
        for j in facts["columns"][c]:  # a row sum or a column sum itself differs, in its last bits
            a, b = pm.chain_sums(d, j, (0, 1)), pm.chain_sums(d, j, (1, 0))
            assert a != b and max(abs(a[0] - b[0]), abs(a[1] - b[1])) <= 4 * np.spacing(max(a))


def test_argmin_placements():
    csr, facts, _, _ = pc.case("argmin_waves")
    rep, tot = c_oracle.medoid(csr, tol=pc.TOL, with_totals=True)
    seen = set()
    for c, where in facts["where"].items():
        t = _cluster_totals(csr, tot, c)
        assert len(t) == facts["n"][c]
        assert tuple(np.flatnonzero(t == t.min())) == where
        assert rep[c] == csr.cluster_off[c] + where[0]
        assert tm.argmin_waves(t) == where[0]
        seen.add((facts["n"][c], where))
    assert seen == {(n, w) for n in (40, 50) for w in ((36,), (5, 36), (32,))}


def test_empties_and_shared_bin_past_32():
    csr, facts, _, _ = pc.case("empties_past_32")
    lens = np.diff(csr.spec_off)
    _, tot = c_oracle.medoid(csr, tol=pc.TOL, with_totals=True)
    assert sorted(facts["empty"].values()) == [(0,), (0, 31, 32, 49), (31,), (32,), (49,)]
    for c, where in facts["empty"].items():
        s0, n = csr.cluster_off[c], csr.cluster_off[c + 1] - csr.cluster_off[c]
        assert n == 50 and [j for j in range(n) if lens[s0 + j] == 0] == sorted(where)
        for j in where:  # d = 1.0 to every spectrum, itself (row and column) included
            assert _cluster_totals(csr, tot, c)[j] == (n + 1) / n
    c = facts["shared"]
    assert csr.cluster_off[c + 1] - csr.cluster_off[c] == 40
    for s in range(csr.cluster_off[c], csr.cluster_off[c + 1]):
        mz = csr.mz[csr.spec_off[s]:csr.spec_off[s + 1]]
        assert len(np_oracle.xcorr_bins(mz, pc.TOL)) == len(mz) - 1  # d(i, i) = 1 - (p - 1)/p > 0


def test_stale_handoff_sequence():
    csr, facts, _, _ = pc.case("stale_handoff")
    assert csr.n_clusters == 9 and csr.n_clusters % 2 == 1
    sizes = np.diff(csr.cluster_off)
    assert tuple(sizes[c] for c in sorted(facts["sizes"])) == pc.STALE_SIZES == (50, 8, 33, 2, 50, 32, 41)
    for c in range(csr.n_clusters):
        assert fc.fits_register_path(csr, c, pc.TOL) == (c not in facts["early"])
    assert len(facts["early"]) == 2 and all(0 < c < csr.n_clusters - 1 for c in facts["early"])
    for c in facts["early"]:  # leaves at run time: a medoid bin past the 32,768-bin table
        assert np_oracle.xcorr_bins(fc.cluster_mz(csr, c), pc.TOL).max() >= fc.MD_BINS


def test_diagonal_content_sits_in_the_first_or_last_columns():
    csr, facts, _, _ = pc.case("diagonal")
    want = sorted((n, kw) for kw in (1, 27) for n in (2, 17, 32))
    assert sorted(zip(facts["n"].values(), facts["KW"].values())) == want
    for c in range(csr.n_clusters):
        n, kw, K = facts["n"][c], facts["KW"][c], facts["K"][c]
        union = np_oracle.xcorr_bins(fc.cluster_mz(csr, c), pc.TOL)
        assert len(union) == K and _kw(K) == kw
        spectra = [m for (m, _i) in csr.cluster(c)]
        assert len(spectra) == n
        # only the two-spectrum clusters of 27 row words are too long for the fused register path
        assert fc.fits_register_path(csr, c, pc.TOL) == (not (n == 2 and kw == 27))
        for s, kind in facts["narrow"][c].items():
            cols = np.searchsorted(union, np_oracle.xcorr_bins(spectra[s], pc.TOL))  # the kernel's columns
            assert np.all(cols < 32) if kind == "first" else np.all(cols >= K - 32)
        kinds = set(facts["narrow"][c].values())
        assert kinds == ({"first", "last"} if n > 2 else set())
        d = pc.distances(csr, c)
        # off the diagonal the counts differ from both diagonal counts somewhere
        assert any(d[i, j] != d[i, i] and d[i, j] != d[j, j] for i in range(n) for j in range(i + 1, n))
