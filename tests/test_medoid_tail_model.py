"""The register tail's summation order (tests/medoid_tail_model.py) against numpy's, on the
host: for every cluster size 2..64 and every column, the row and column sums the lane pair
forms equal np.add.reduce on the reference's dense upper-triangular matrix bit for bit, and
the argmin takes the lowest index among equal totals."""
import numpy as np
import pytest

import medoid_tail_model as m

SIZES = list(range(2, 65))


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _random_d(n, rng):
    """Symmetric distances 1 - c/q as the kernel meets them (a wide spread of mantissas)."""
    q = rng.integers(1, 300, (n, n))
    q = np.minimum(q, q.T)
    c = (rng.random((n, n)) * (q + 1)).astype(np.int64)
    c = np.minimum(np.triu(c) + np.triu(c, 1).T, q)
    return 1.0 - c / q


def _tied_d(n, rng):
    """Matrices full of ties: distances from {0, 1/3, 1/2, 2/3, 1}."""
    v = np.array([0.0, 1.0 - 2.0 / 3.0, 0.5, 1.0 - 1.0 / 3.0, 1.0])
    a = v[rng.integers(0, len(v), (n, n))]
    return np.triu(a) + np.triu(a, 1).T


def test_walk_covers_every_row_once_in_numpy_order():
    for n in SIZES:
        w = m.lane_walk(n, 0)
        lim = w["lim"]
        assert lim == (n - n % 8 if n >= 8 else 0)
        for fh in (0, 1):
            for i in range(4):
                k = 4 * fh + i
                assert w["acc"][(fh, i)] == list(range(k, lim, 8))  # r[k]: k, k + 8, ... ascending
        assert w["tail"][0] + w["tail"][1] == list(range(lim, n))


@pytest.mark.parametrize("maker", [_random_d, _tied_d], ids=["random", "ties"])
def test_sums_equal_numpy_bit_for_bit(maker):
    rng = np.random.default_rng(11)
    for n in SIZES:
        d = maker(n, rng)
        assert np.array_equal(d, d.T)
        ref = m.reference_sums(d)
        for j in range(n):
            row, col = m.column_sums(d, j)
            assert _bits(row) == _bits(ref[j][0]), (n, j, "row")
            assert _bits(col) == _bits(ref[j][1]), (n, j, "col")
        t = m.totals(d)
        want = m.reference_totals(d)
        assert np.array_equal(_bits(t), _bits(want)), n
        assert m.argmin_waves(t) == int(np.flatnonzero(want == want.min())[0]), n


def test_all_equal_totals_pick_index_zero():
    for n in SIZES:
        assert m.argmin_waves(np.full(n, 0.75)) == 0


@pytest.mark.parametrize("lo,hi,n", [(5, 40, 50), (0, 32, 33), (31, 32, 64), (3, 63, 64), (40, 41, 50), (33, 50, 51)])
def test_tie_between_and_within_waves_picks_the_lower(lo, hi, n):
    t = np.full(n, 0.9)
    t[[lo, hi]] = 0.25
    assert m.argmin_waves(t) == lo
    t[lo] = 0.5  # the higher index alone holds the minimum now
    assert m.argmin_waves(t) == hi
