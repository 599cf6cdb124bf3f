"""A numpy model of medoid_tail_regs (specpride_amd/csrc/medoid.hip): the lane / tile walk
that turns the MFMA accumulator into the medoid's totals without a distance matrix in LDS.

The kernel's facts the model restates:

* wave w (0, and 1 for n > 32) owns columns 32w..32w+31; it walks row tile 0, then (n > 32)
  row tile 1; the 32 x 32 C/D layout gives lane (j = lane & 31, fh = lane >> 5) column j at
  rows (q & 3) + 8 * (q >> 2) + 4 * fh, q = 0..15
* lim = n - n % 8 (0 for n < 8); a group of eight rows starting below lim is added into four
  row-sum and four column-sum accumulators per lane (index mod 8 = 4 * fh + (q & 3)), with
  +0.0 in place of the terms on the other side of the diagonal
* each half combines (a0 + a1) + (a2 + a3); one exchange, one add
* the tail rows lim..n-1 are added one by one: lim..lim+3 in the fh = 0 lane, the sum is
  handed over once, lim+4.. in the fh = 1 lane; then 0.0 + sum and (row + col) / n
* the argmin takes the lowest index among equal totals; wave 1's minimum replaces wave 0's
  only if it is strictly smaller

``d`` is the full symmetric distance matrix d[r, j] = d[j, r] (the MFMA computes both
triangles); the reference sums the rows and columns of its upper triangle (diagonal included,
zeros below: most_similar_representative.py:91-100).
"""
import numpy as np


def tile_rows(fh):
    """Rows of a 32-row tile that half fh of the wave holds, in accumulator order q = 0..15."""
    return [(q & 3) + 8 * (q >> 2) + 4 * fh for q in range(16)]


def lane_walk(n, j):
    """The order in which column j's lane pair meets the row indices: a dict with
    'acc': {(fh, i): [r, ...]} the rows added into accumulator i of half fh, in order;
    'tail': ([rows added in fh = 0], [rows added in fh = 1]) of the sequential tail."""
    lim = n - n % 8 if n >= 8 else 0
    acc = {(fh, i): [] for fh in (0, 1) for i in range(4)}
    for t in range(2 if n > 32 else 1):
        for fh in (0, 1):
            rows = tile_rows(fh)
            for g in range(4):
                if t * 32 + 8 * g < lim:
                    for i in range(4):
                        acc[(fh, i)].append(t * 32 + rows[4 * g + i])
    tail = ([r for r in range(lim, lim + 4) if r < n], [r for r in range(lim + 4, lim + 8) if r < n])
    return {"acc": acc, "tail": tail, "lim": lim}


def column_sums(d, j):
    """(row sum j, column sum j) as the lane pair of column j forms them, f64 step by step."""
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    walk = lane_walk(n, j)
    zero = np.float64(0.0)
    out = []
    for keep in (lambda r: r >= j, lambda r: r <= j):  # the row sum's terms, the column sum's
        half = []
        for fh in (0, 1):
            a = [zero] * 4
            for i in range(4):
                for r in walk["acc"][(fh, i)]:
                    a[i] = a[i] + (d[r, j] if keep(r) else zero)
            half.append((a[0] + a[1]) + (a[2] + a[3]))
        s = half[0] + half[1]
        for r in walk["tail"][0]:  # fh = 0
            s = s + (d[r, j] if keep(r) else zero)
        for r in walk["tail"][1]:  # handed over to fh = 1
            s = s + (d[r, j] if keep(r) else zero)
        out.append(zero + s)
    return out[0], out[1]


def totals(d):
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    t = np.empty(n, np.float64)
    for j in range(n):
        row, col = column_sums(d, j)
        t[j] = (row + col) / np.float64(n)
    return t


def argmin_waves(t):
    """The kernel's P6: per wave (columns 0..31, 32..63) the lowest index of the minimum by
    an xor butterfly over 64 lanes (finished totals sit in lanes 32..63, the others hold
    +inf), then wave 1's result taken only if strictly smaller."""
    t = np.asarray(t, np.float64)
    n = len(t)
    res = []
    for w in range(2 if n > 32 else 1):
        best = [np.inf] * 64
        idx = [0x7FFFFFFF] * 64
        for fr in range(32):
            j = 32 * w + fr
            if j < n:
                best[32 + fr], idx[32 + fr] = t[j], j
        o = 32
        while o:
            nb, ni = list(best), list(idx)
            for lane in range(64):
                t2, i2 = best[lane ^ o], idx[lane ^ o]
                if t2 < best[lane] or (t2 == best[lane] and i2 < idx[lane]):
                    nb[lane], ni[lane] = t2, i2
            best, idx = nb, ni
            o >>= 1
        res.append((best[0], idx[0]))
    b, i = res[0]
    if len(res) == 2 and res[1][0] < b:
        b, i = res[1]
    return i


def reference_totals(d):
    """most_similar_representative.py:91-100 on the dense upper-triangular matrix."""
    D = np.triu(np.asarray(d, np.float64))
    n = D.shape[0]
    return np.array([(np.add.reduce(D[i, :]) + np.add.reduce(D[:, i])) / n for i in range(n)])


def reference_sums(d):
    D = np.triu(np.asarray(d, np.float64))
    n = D.shape[0]
    return [(np.add.reduce(D[i, :]), np.add.reduce(D[:, i])) for i in range(n)]
