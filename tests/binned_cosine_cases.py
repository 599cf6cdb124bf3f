"""Named inputs of the binned-cosine evaluation (spx_binned_cosine) at the branches of
csrc/binned_cosine.hip that ordinary spectra never take: a representative on the
rightmost edge, bins past the bucket table, runs of equal bins at the 64-peak chunk
boundaries, an invalid peak between two peaks of one bin, more deferred clusters
than fallback workgroups, representative lengths at the LDS cap, other bin widths,
and non-finite intensities.

A case is a list of ``(members, representative)`` clusters, a spectrum a pair of
``(mz, intensity)`` arrays.  ``expect(name)`` is ``oracle/np_oracle.binned_cosine``
on it, computed once per process; ``tests/golden/binned_cosine_edges.npz`` pins the
same cases to the reference's own ``benchmark.cos_dist`` / ``average_cos_dist``
(make_golden_binned_cosine_edges.py), and tests/test_binned_cosine_inputs.py checks
that every case has the property it is named for.
"""
import numpy as np

from oracle import np_oracle
from specpride_amd.csr import SpectraCSR

MZ_SPACE = np_oracle.MZ_SPACE
STATUS_OK, STATUS_EMPTY, STATUS_UNRESOLVED = 0, 3, 100
RTOL = 1e-12          # tests/test_gpu_cosine.py: BLAS summation-order differences
WAVE = 64             # peaks of a member per chunk (kWave)
RCAP = 512            # SPX_CS_RCAP (csrc/binned_cosine.hip): representative peaks held in LDS
FALLBACK_BLOCKS = 64  # kFallbackBlocks (csrc/spx_api.hip): workgroups of the global-scratch kernel
TABLE_BINS = 1 << 19  # bins below this are looked up through the bucket table (CS_BMAX << CS_BSH)
SPACINGS = (0.005, 0.02, 0.1, 1.0005)
INF, NAN = np.inf, np.nan


def edge(i, s=MZ_SPACE):
    """np.arange(-s/2, stop, s)[i] as numpy's DOUBLE_fill writes it."""
    start = -s / 2.
    return start if i == 0 else (start + s if i == 1 else start + i * ((start + s) - start))


def n_edges(max_mz, s=MZ_SPACE):
    """len(np.arange(-s/2, max_mz, s))."""
    return int(np.ceil((max_mz - (-s / 2.)) / s))


def last_edge(max_mz, s=MZ_SPACE):
    return edge(n_edges(max_mz, s) - 1, s)


def decimals(s=MZ_SPACE):
    """The decimals scipy's on-edge test rounds to (a nominal edge gap of s)."""
    return int(-np.log10(s)) + 6


def mid(b, s=MZ_SPACE, frac=0.5):
    """An m/z inside bin b, ``frac`` of the way from its left edge."""
    return edge(b, s) + frac * s


def _a(*x):
    return np.array(x, np.float64)


def _spec(mz, it):
    return np.asarray(mz, np.float64), np.asarray(it, np.float64)


# ------------------------------------------------------------------ rep_on_edge
def _on_edge_offsets(s):
    u = 10.0 ** -decimals(s)
    return 0.1 * u, 0.3 * u, 20 * u  # two that round onto the edge, one that does not


def _roe_rep(M, s, kc_peak, order=None):
    e = last_edge(M, s)
    o1, o2, o3 = _on_edge_offsets(s)
    mz = [100.001, 700.501] + ([e - 0.4 * s] if kc_peak else []) + [e + o1, e + o2, e + o3]
    it = [10.0, 20.0] + ([30.0] if kc_peak else []) + [40.0, 50.0, 60.0]
    mz, it = np.array(mz), np.array(it)
    if order is not None:
        mz, it = mz[list(order)], it[list(order)]
    return mz, it


def _roe_mem(M, s, kc_peak):
    e = last_edge(M, s)
    mz = [100.0, 700.5] + ([e - 0.6 * s] if kc_peak else []) + [M]
    it = [1.0, 2.0] + ([3.0] if kc_peak else []) + [4.0]
    return np.array(mz), np.array(it)


ROE_VARIANTS = ("a", "b", "c", "d", "e", "f_a", "f_e")


def case_rep_on_edge(s=MZ_SPACE):
    M, MF = 1500.0, 3200.0
    a = ([_roe_mem(M, s, False)], _roe_rep(M, s, True))
    b = ([_roe_mem(M, s, False)], _roe_rep(M, s, False))
    c = ([_roe_mem(M, s, False), _roe_mem(M, s, True)], _roe_rep(M, s, True, order=(4, 0, 2, 3, 1, 5)))
    far = _spec([100.0, 700.5, last_edge(M, s) + 0.5 * s, M + 50.0], [1.0, 2.0, 5.0, 4.0])
    d = ([_roe_mem(M, s, True), far], _roe_rep(M, s, True))
    e = ([_roe_mem(M, s, True)], _roe_rep(M, s, True))
    f_a = ([_roe_mem(MF, s, False)], _roe_rep(MF, s, True))
    f_e = ([_roe_mem(MF, s, True)], _roe_rep(MF, s, False))
    return [a, b, c, d, e, f_a, f_e]


# ---------------------------------------------------------------------- high_mz
HIGH_SEAM = (TABLE_BINS - 2, TABLE_BINS - 1, TABLE_BINS, TABLE_BINS + 1)


def _bins_spec(rng, bins, s=MZ_SPACE, per_bin=None):
    """One peak mid-bin per entry of ``bins`` (in that order); ``per_bin`` adds a second
    peak to some of them, right after the first."""
    mz = []
    for k, b in enumerate(bins):
        mz.append(mid(int(b), s))
        if per_bin is not None and per_bin[k]:
            mz.append(mid(int(b), s, 0.7))
    mz = np.array(mz)
    return mz, np.round(rng.uniform(1.0, 100.0, len(mz)), 3)


def case_high_mz():
    rng = np.random.default_rng(2101)
    s = MZ_SPACE
    lo, hi = int(3000.0 / s), int(4500.0 / s)
    out = []
    for k in range(3):
        high = np.sort(rng.choice(np.arange(lo, hi), 24, replace=False))
        low = np.sort(rng.choice(np.arange(int(150.0 / s), int(2600.0 / s)), 20, replace=False))
        pool = np.concatenate([low, HIGH_SEAM, high])  # ascending
        top = pool[-1]
        members = []
        for j in range(4):
            keep = rng.random(len(pool)) < 0.7
            keep[len(low):len(low) + 4] = True   # the seam bins
            keep[len(low) + 1] = j != 1          # ... but one member lacks bin 524,287
            keep[-1] = j % 2 == 0                # two members end below the representative's last peak
            members.append(_bins_spec(rng, pool[keep], per_bin=rng.random(int(keep.sum())) < 0.2))
            assert len(members[-1][0]) <= 70
        rkeep = rng.random(len(pool)) < 0.7
        rkeep[len(low):len(low) + 4] = True
        rkeep[-1] = True
        if k == 0:    # <= RCAP peaks, sorted, lacks bin 524,288
            rkeep[len(low) + 2] = False
            rep = _bins_spec(rng, pool[rkeep], per_bin=rng.random(int(rkeep.sum())) < 0.3)
        elif k == 1:  # unsorted: the last peak in input order is not the largest
            rb = pool[rkeep]
            p = rng.permutation(len(rb))
            while rb[p[-1]] == top:
                p = rng.permutation(len(rb))
            rep = _bins_spec(rng, rb[p])
        else:         # > RCAP peaks: the global-scratch kernel, the same lookup
            extra = rng.choice(np.setdiff1d(np.arange(int(150.0 / s), hi), pool), 600 - int(rkeep.sum()), replace=False)
            rep = _bins_spec(rng, np.sort(np.concatenate([pool[rkeep], extra])))
            assert len(rep[0]) > RCAP
        out.append((members, rep))
    return out


# ------------------------------------------------------------------- chunk_runs
# per member: (length, first position of the run, its length)
CHUNK_RUNS = ((150, 10, 130), (80, 60, 4), (141, 120, 8), (140, 64, 64), (64, 60, 4), (128, 120, 8), (65, 60, 5))


def _run_member(rng, n, r0, rl, b0, s=MZ_SPACE):
    """n peaks in ascending bins from b0, 7 bins apart, positions [r0, r0 + rl) in one bin."""
    bins, b = [], b0
    for q in range(n):
        if not (r0 < q < r0 + rl):
            b += 7
        bins.append(b)
    fr = np.array([0.2 + 0.6 * ((q - r0) / rl if r0 <= q < r0 + rl else 0.5) for q in range(n)])
    mz = np.array([mid(bb, s, f) for bb, f in zip(bins, fr)])
    it = rng.permutation(n).astype(np.float64) + 1.0 + np.round(rng.random(n), 3)  # distinct
    return mz, it


def case_chunk_runs():
    rng = np.random.default_rng(2102)
    s = MZ_SPACE
    b0 = int(200.0 / s)
    members = [_run_member(rng, n, r0, rl, b0) for n, r0, rl in CHUNK_RUNS]
    # the representative: every member's run bin (they share b0 + 7 * (r0 + 1)) and a few others
    rb = sorted({b0 + 7 * (r0 + 1) for _, r0, _ in CHUNK_RUNS} | {b0 + 7 * k for k in (1, 5, 30, 70, 100, 135)})
    rep_mz = np.array([mid(b, s) for b in rb] + [1000.0])
    rep = (rep_mz, np.round(rng.uniform(1.0, 50.0, len(rep_mz)), 3))
    return [(members, rep)]


# ------------------------------------------------------------------- sandwiched
# per member: (position of the invalid peak, kind); the equal bins sit right before and after
SANDWICHED = ((1, "above"), (1, "below"), (11, "above"), (11, "below"), (64, "above"), (64, "below"),
              (63, "above"), (63, "below"), (1, "nan"))
SANDWICH_REP_LAST = 1500.0


def _sandwich_member(rng, pos, kind, s=MZ_SPACE):
    bad = {"above": 1999.0, "below": -1.0, "nan": NAN}[kind]
    if pos == 1:
        if kind == "above":
            return _a(500.0, 1999.0, 500.001, 1000.0), _a(3.0, 100.0, 5.0, 2.0)
        return _a(500.0, bad, 500.001, 1000.0), _a(3.0, 100.0, 5.0, 2.0)
    n = pos + 6
    b0 = int(300.0 / s)
    mz = np.array([mid(b0 + 9 * q, s) for q in range(n)])
    mz[pos] = bad
    mz[pos + 1] = mid(b0 + 9 * (pos - 1), s, 0.7)  # the bin of the peak before the invalid one
    it = rng.permutation(n).astype(np.float64) + 1.0 + np.round(rng.random(n), 3)
    return mz, it


def case_sandwiched():
    rng = np.random.default_rng(2103)
    s = MZ_SPACE
    members = [_sandwich_member(rng, pos, kind) for pos, kind in SANDWICHED]
    b0 = int(300.0 / s)
    rb = [b0 + 9 * q for q in (0, 10, 30, 62, 63, 66)] + [int(500.0 / s + 0.5)]
    rep_mz = np.sort(np.array([mid(b, s) for b in rb] + [SANDWICH_REP_LAST]))
    return [(members, (rep_mz, np.round(rng.uniform(1.0, 50.0, len(rep_mz)), 3)))]


# ---------------------------------------------------------------- many_deferred
N_DEFERRED_CLUSTERS = 72


def _dense_peaks(rng, R, lo=100.0, hi=300.0):
    return np.sort(np.round(rng.uniform(lo, hi, R), 3)), np.round(rng.lognormal(4, 1, R), 1)


def _members_of(rng, rep_mz, n, k=20, last=None):
    out = []
    for _ in range(n):
        mz = np.sort(np.round(rng.choice(rep_mz, k, replace=False) + rng.normal(0, 0.002, k), 4))
        if last is not None:
            mz = np.append(mz, last)
        out.append((mz, np.round(rng.lognormal(5, 1, len(mz)), 1)))
    return out


def case_many_deferred():
    rng = np.random.default_rng(2104)
    out = []
    for c in range(N_DEFERRED_CLUSTERS):
        R = 640 - (c * 127) // (N_DEFERRED_CLUSTERS - 1)  # 640 down to 513
        mz, it = _dense_peaks(rng, R)
        members = _members_of(rng, mz, 2)
        if c % 10 == 5:  # unsorted: the rank sort in the scratch slice
            p = rng.permutation(R)
            mz, it = mz[p], it[p]
        if c == 30:
            members = []
        if c == 40:
            members[1] = (np.zeros(0), np.zeros(0))
        out.append((members, (mz, it)))
    return out


# ---------------------------------------------------------------- rcap_boundary
RCAP_LENGTHS = (RCAP - 1, RCAP, RCAP + 1)


def case_rcap_boundary():
    rng = np.random.default_rng(2105)
    mz, it = _dense_peaks(rng, RCAP + 1)
    members = _members_of(rng, mz[:RCAP - 1], 3, last=320.0)  # the members set the cut: the same for all three
    return [(members, (mz[:R].copy(), it[:R].copy())) for R in RCAP_LENGTHS]


# --------------------------------------------------------------------- mz_space
def case_mz_space(s):
    rng = np.random.default_rng(2106)
    t = np.sort(rng.uniform(100.0, 500.0, 15))
    members = [(np.round(np.sort(t + rng.normal(0, 0.3 * s, 15)), 6), np.round(rng.lognormal(5, 1, 15), 2)) for _ in range(3)]
    rep = (np.round(np.sort(t + rng.normal(0, 0.3 * s, 15)), 6), np.round(rng.lognormal(5, 1, 15), 2))
    M = 900.0
    e = last_edge(M, s)
    o1, o2, o3 = _on_edge_offsets(s)
    on_mem = _spec([100.001, 700.501, e, e + o2, e + o3], [1.0, 2.0, 3.0, 4.0, 5.0])
    on_mem_rep = _spec([100.0, 700.5, e - 0.5 * s, M], [10.0, 20.0, 30.0, 40.0])
    return [(members, rep), ([on_mem], on_mem_rep), ([_roe_mem(M, s, True)], _roe_rep(M, s, True))]


# -------------------------------------------------------------------- nonfinite
def case_nonfinite():
    rng = np.random.default_rng(2107)
    plain = _spec([200.0, 300.0], [1.0, 1.0])
    zero = _spec([200.0, 300.0], [0.0, 0.0])
    out = [
        ([plain], _spec([100.0, 200.0], [INF, 1.0])),                 # 0 inf in a bin the member lacks
        ([plain], _spec([100.0, 200.0], [1.0, INF])),                 # 1 inf in a shared bin
        ([plain], _spec([100.0, 200.0, 400.0], [1.0, 1.0, INF])),     # 2 inf past the representative's own cut
        ([plain], _spec([100.0, 400.0, 200.0], [1.0, INF, 1.0])),     # 3 inf past the member's cut (unsorted)
        ([_spec([200.0, 300.0], [INF, 1.0]), _spec([150.0, 200.0, 300.0], [INF, 1.0, 1.0]),
          _spec([200.0, 300.0], [-INF, 1.0])], _spec([100.0, 200.0], [1.0, 1.0])),  # 4 the member's inf: shared, unshared
        ([plain], _spec([100.0, 100.001, 200.0], [INF, -INF, 1.0])),  # 5 +inf and -inf in one bin
        ([_spec([200.0, 200.001, 300.0], [INF, -INF, 1.0]), plain], _spec([100.0, 200.0], [1.0, 1.0])),
        ([plain], _spec([100.0, 200.0], [NAN, 1.0])),                 # 7 NaN intensity
        ([_spec([200.0, 300.0], [NAN, 1.0]), _spec([150.0, 300.0], [NAN, 1.0])], _spec([100.0, 200.0], [1.0, 1.0])),
        ([zero, plain], _spec([100.0, 200.0], [INF, 1.0])),           # 9 inf against an all-zero partner: 0.0
        ([_spec([200.0, 300.0], [INF, 1.0])], _spec([100.0, 200.0], [0.0, 0.0])),
        ([plain], _spec([100.0, 200.0], [1e200, 1.0])),               # 11 the square overflows, no bin is infinite: 0.0
        ([_spec([200.0, 250.0, 300.0], [1.0, 1e200, 1.0])], _spec([100.0, 200.0], [1.0, 1.0])),
        ([plain], _spec([100.0, 200.0, 400.0], [1.0, 1.0, 1e200])),   # 13 ... and past the cut it changes nothing
        ([plain], _spec([100.0, 100.001, 200.0], [1e308, 1e308, 1.0])),  # 14 finite peaks, an infinite bin sum
        ([_spec([150.0, 150.001, 200.0, 300.0], [1e308, 1e308, 1.0, 1.0])], _spec([100.0, 200.0], [1.0, 1.0])),
    ]
    # 16: the on-edge sum is infinite (the run of bin kc itself is finite)
    M = 1500.0
    rm, ri = _roe_rep(M, MZ_SPACE, True)
    ri = ri.copy()
    ri[3] = INF
    out.append(([_roe_mem(M, MZ_SPACE, False)], (rm, ri)))
    # 17: members longer than a chunk -- inf in a run carried across position 64, inf in an
    # unsorted member, and the same members without it
    n, r0, rl = 80, 60, 8
    mz, it = _run_member(rng, n, r0, rl, int(200.0 / MZ_SPACE))
    hot = it.copy()
    hot[62] = INF
    p = rng.permutation(n)
    rep17 = _spec([mid(int(200.0 / MZ_SPACE) + 7 * k) for k in (1, 5, 61)] + [900.0], [3.0, 4.0, 5.0, 6.0])
    out.append(([(mz, hot), (mz, it), (mz[p], hot[p]), (mz[p], it[p])], rep17))
    # 18, 19: a representative past the LDS cap with inf inside the cut and past it
    dm, di = _dense_peaks(rng, RCAP + 8)
    members = _members_of(rng, dm, 2, last=250.0)
    inside, past = di.copy(), di.copy()
    inside[int(np.searchsorted(dm, 180.0))] = INF
    past[-1] = INF  # the representative's own last peak lies past every cut
    out.append((members, (dm, inside)))
    out.append((members, (dm, past)))
    return out


# ------------------------------------------------------------------- unresolved
UNRESOLVED_MAX_REP = 600
UNRESOLVED_LENGTHS = (40, 513, 700, 300, 560)


def case_unresolved():
    """One representative longer than the caller's max_rep_peaks (600) among ordinary
    and 513-peak ones; the oracle scores all of them."""
    rng = np.random.default_rng(2108)
    out = []
    for R in UNRESOLVED_LENGTHS:
        mz, it = _dense_peaks(rng, R)
        out.append((_members_of(rng, mz, 2), (mz, it)))
    return out


CASES = {
    "rep_on_edge": (case_rep_on_edge, MZ_SPACE), "high_mz": (case_high_mz, MZ_SPACE),
    "chunk_runs": (case_chunk_runs, MZ_SPACE), "sandwiched": (case_sandwiched, MZ_SPACE),
    "many_deferred": (case_many_deferred, MZ_SPACE), "rcap_boundary": (case_rcap_boundary, MZ_SPACE),
    "nonfinite": (case_nonfinite, MZ_SPACE), "unresolved": (case_unresolved, MZ_SPACE),
}
CASES.update({f"mz_space_{s}": ((lambda s=s: case_mz_space(s)), s) for s in SPACINGS})

_cache = {}


def clusters_of(name):
    if name not in _cache:
        _cache[name] = {"clusters": CASES[name][0]()}
    return _cache[name]["clusters"]


def mz_space_of(name):
    return CASES[name][1]


def to_csr(name):
    """(members as a SpectraCSR, rep_off, rep_mz, rep_int) of a named case."""
    cl = clusters_of(name)
    csr = SpectraCSR.from_clusters([[{"m/z array": np.asarray(m, np.float64), "intensity array": np.asarray(i, np.float64)}
                                     for m, i in members] for members, _ in cl])
    rep_off = np.zeros(len(cl) + 1, np.int64)
    np.cumsum([len(rep[0]) for _, rep in cl], out=rep_off[1:])
    rep_mz = np.concatenate([np.asarray(rep[0], np.float64) for _, rep in cl])
    rep_int = np.concatenate([np.asarray(rep[1], np.float64) for _, rep in cl])
    return csr, rep_off, rep_mz, rep_int


def expect(name):
    """(cos [S], avg [C], status [C]) of the numpy oracle, computed once per process."""
    clusters_of(name)
    if "expect" not in _cache[name]:
        with np.errstate(invalid="ignore", over="ignore"):  # the non-finite cases: the reference's own arithmetic
            _cache[name]["expect"] = np_oracle.binned_cosine(*to_csr(name), mz_space_of(name))
    return _cache[name]["expect"]


def golden_case(z, name):
    """Slice one case out of tests/golden/binned_cosine_edges.npz:
    (csr, rep_off, rep_mz, rep_int, mz_space, (cos, avg, status))."""
    k = list(z["case_names"]).index(name)
    c0, c1 = int(z["case_off"][k]), int(z["case_off"][k + 1])
    s0, s1 = int(z["cluster_off"][c0]), int(z["cluster_off"][c1])
    p0, p1 = int(z["spec_off"][s0]), int(z["spec_off"][s1])
    r0, r1 = int(z["rep_off"][c0]), int(z["rep_off"][c1])
    csr = SpectraCSR(z["cluster_off"][c0:c1 + 1] - s0, z["spec_off"][s0:s1 + 1] - p0, z["mz"][p0:p1], z["inten"][p0:p1],
                     z["prec_mz"][s0:s1], z["charge"][s0:s1], z["rt"][s0:s1])
    want = (z["cos"][s0:s1], z["avg"][c0:c1], z["status"][c0:c1])
    return csr, z["rep_off"][c0:c1 + 1] - r0, z["rep_mz"][r0:r1], z["rep_int"][r0:r1], float(z["case_mz_space"][k]), want
