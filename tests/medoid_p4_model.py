"""The register tail past 32 spectra, one Gram tile per wave (medoid_tail_regs,
specpride_amd/csrc/medoid.hip): tests/medoid_tail_model.py's lane walk extended to the
hand-off between the two waves of a column tile.

What the kernel does for column j (column tile ct = j // 32) of a cluster of n > 32 spectra:

* the row-tile-0 wave starts the four row-sum and four column-sum accumulators of each lane
  half at +0.0 and adds the four groups of eight rows 0..31 (all below lim, which is >= 32)
* what crosses, per lane half:
    ct = 0  the four row-sum accumulators; the column sum is complete (rows 32.. lie below
            the diagonal of every column 0..31), so the wave combines it -- (a0 + a1) +
            (a2 + a3) per half, one exchange, one add -- and hands over the finished value
    ct = 1  the four column-sum accumulators (rows 0..31 lie above the diagonal of every
            column 32..63: they add to the column sums only); the row sums start at +0.0
* the row-tile-1 wave goes on with the groups of rows 32.. that start below lim, combines,
  takes the handed-over column sum for ct = 0, adds the tail rows lim..n-1 one by one
  (tests/medoid_tail_model.py), then 0.0 + sum and (row + col) / n
* the finishing waves are waves 0 and 1 (columns 0..31 and 32..63), so the argmin is
  medoid_tail_model.argmin_waves unchanged

``tile_order`` = (1, 0) is the wrong kernel that adds row tile 1's terms into each
accumulator before row tile 0's: tests use it to prove a case is sensitive to the order.
"""
import numpy as np

import medoid_tail_model as tm

ZERO = np.float64(0.0)


def _keep_row(r, j):
    return r >= j


def _keep_col(r, j):
    return r <= j


def _fold(a, d, j, t, lim, keep):
    """Adds row tile t's groups below lim into a[fh][i], in the accumulator's order."""
    for fh in (0, 1):
        rows = tm.tile_rows(fh)
        for g in range(4):
            if t * 32 + 8 * g < lim:
                for i in range(4):
                    r = t * 32 + rows[4 * g + i]
                    a[fh][i] = a[fh][i] + (d[r, j] if keep(r, j) else ZERO)


def _combine(a):
    half = [(a[fh][0] + a[fh][1]) + (a[fh][2] + a[fh][3]) for fh in (0, 1)]
    return half[0] + half[1]


def crossing(ct):
    """Which accumulators cross the hand-off of column tile ct, and whether the finished
    column sum does."""
    return dict(row_acc=ct == 0, col_acc=ct == 1, col_sum=ct == 0)


def handoff_sums(d, j, tile_order=(0, 1)):
    """(row sum j, column sum j) of a cluster of n > 32 spectra as the two waves of column
    tile j // 32 form them, f64 step by step."""
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    assert n > 32
    lim = n - n % 8
    ct = j // 32
    first, second = tile_order
    # the first wave
    ra = [[ZERO] * 4, [ZERO] * 4]
    ca = [[ZERO] * 4, [ZERO] * 4]
    _fold(ra, d, j, first, lim, _keep_row)
    _fold(ca, d, j, first, lim, _keep_col)
    cross = crossing(ct)
    cs_done = _combine(ca) if cross["col_sum"] else None
    # the second wave: what did not cross starts at +0.0 again
    ra2 = [list(h) for h in ra] if cross["row_acc"] else [[ZERO] * 4, [ZERO] * 4]
    ca2 = [list(h) for h in ca] if cross["col_acc"] else [[ZERO] * 4, [ZERO] * 4]
    _fold(ra2, d, j, second, lim, _keep_row)
    _fold(ca2, d, j, second, lim, _keep_col)
    rs = _combine(ra2)
    cs = cs_done if cross["col_sum"] else _combine(ca2)
    for r in range(lim, n):  # the sequential tail: fh = 0's rows, handed over, fh = 1's
        rs = rs + (d[r, j] if _keep_row(r, j) else ZERO)
        cs = cs + (d[r, j] if _keep_col(r, j) else ZERO)
    return ZERO + rs, ZERO + cs


def handoff_totals(d, tile_order=(0, 1)):
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    t = np.empty(n, np.float64)
    for j in range(n):
        row, col = handoff_sums(d, j, tile_order)
        t[j] = (row + col) / np.float64(n)
    return t


def chain_sums(d, j, tile_order=(0, 1)):
    """The same sums with every term added, none replaced by a hand-off rule: each
    accumulator takes the groups of tile_order[0], then of tile_order[1].  With (0, 1) this
    is medoid_tail_model.column_sums; handoff_sums must equal it bit for bit (the +0.0 rule)."""
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    lim = n - n % 8
    out = []
    for keep in (_keep_row, _keep_col):
        a = [[ZERO] * 4, [ZERO] * 4]
        for t in tile_order:
            _fold(a, d, j, t, lim, keep)
        s = _combine(a)
        for r in range(lim, n):
            s = s + (d[r, j] if keep(r, j) else ZERO)
        out.append(ZERO + s)
    return out[0], out[1]
