"""Inputs and the CPU oracle of the cosine medoid (spx_cosine_medoid).

The oracle has two layers.  ``oracle/np_oracle.py`` restates the reference's
``cos_dist`` (benchmark.py:19-29) and is pinned to it by ``binned_cosine.npz``.
The composition lives here, as the issue defines it:

    score[i] = average_cos_dist(member_i, members)      (benchmark.py:31-38:
               s = 0.0; for j in 0..n-1: s += cos_dist(member_i, member_j); s / float(n))
    rep      = the first i with the maximal score (scan from score[0], replace on >)

``cos_dist`` is symmetric bit for bit (np.dot(a, b) == np.dot(b, a), a * b == b * a),
so every unordered pair is evaluated once and mirrored; test_cosine_medoid_inputs.py
checks that on the golden clusters, and ``cosine_medoid.npz`` pins the composition to
the reference's own ``average_cos_dist``.

A cluster is a list of ``(mz, intensity)`` arrays.  Every named case is a list of
clusters; ``expect(name)`` is its oracle result, computed once per process.
"""
import numpy as np

from oracle import np_oracle
from specpride_amd.csr import SpectraCSR
from specpride_amd.synthetic import make_clusters_np

MZ_SPACE = np_oracle.MZ_SPACE
STATUS_OK, STATUS_EMPTY, STATUS_UNRESOLVED = 0, 3, 100
RTOL = 1e-12      # tests/test_gpu_cosine.py: BLAS summation-order differences
TIE_GAP = 1e-9    # best and runner-up are bitwise equal or further apart than this (relative)
LDS_MEMBERS, LDS_RUNS = 64, 11264  # engine.COSINE_MEDOID_LDS_* (checked in test_cosine_medoid_inputs.py)


# ------------------------------------------------------------------ the oracle
def pair_matrix(members, mz_space=MZ_SPACE):
    n = len(members)
    S = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            S[i, j] = S[j, i] = np_oracle.cos_dist(members[i][0], members[i][1], members[j][0], members[j][1], mz_space)
    return S


def scores_and_rep(members, mz_space=MZ_SPACE):
    """(scores [n], rep) of one cluster without empty members (n >= 1)."""
    S = pair_matrix(members, mz_space)
    n = len(members)
    scores = np.zeros(n)
    for i in range(n):
        s = 0.0
        for j in range(n):
            s += S[i, j]
        scores[i] = s / float(n)
    rep = 0
    for i in range(1, n):
        if scores[i] > scores[rep]:
            rep = i
    return scores, rep


def oracle(clusters, mz_space=MZ_SPACE):
    """(rep [C] global spectrum index or -1, score [S], status [C]) as spx_cosine_medoid
    reports them: an empty cluster is OK with rep -1; a cluster with an empty member
    (the reference's mz[-1] raises IndexError) is EMPTY with rep -1 and NaN scores."""
    rep, score, status = [], [], []
    first = 0
    for members in clusters:
        n = len(members)
        if n == 0:
            rep.append(-1)
            status.append(STATUS_OK)
        elif any(len(m[0]) == 0 for m in members):
            rep.append(-1)
            status.append(STATUS_EMPTY)
            score.extend([np.nan] * n)
        else:
            sc, r = scores_and_rep(members, mz_space)
            rep.append(first + r)
            status.append(STATUS_OK)
            score.extend(sc)
        first += n
    return np.array(rep, np.int64), np.array(score, np.float64), np.array(status, np.int32)


def to_csr(clusters) -> SpectraCSR:
    return SpectraCSR.from_clusters([[{"m/z array": np.asarray(m, np.float64), "intensity array": np.asarray(i, np.float64)}
                                      for m, i in cl] for cl in clusters])


def from_csr(csr):
    return [[(csr.mz[csr.spec_off[s]:csr.spec_off[s + 1]].copy(), csr.inten[csr.spec_off[s]:csr.spec_off[s + 1]].copy())
             for s in range(csr.cluster_off[c], csr.cluster_off[c + 1])] for c in range(csr.n_clusters)]


def edge(i, s=MZ_SPACE):
    """np.arange(-s/2, stop, s)[i] as numpy's DOUBLE_fill writes it."""
    start = -s / 2.
    return start if i == 0 else (start + s if i == 1 else start + i * ((start + s) - start))


def ulp_above_edge(near):
    """The double one ulp above the edge nearest to ``near`` m/z."""
    i = int(round((near + MZ_SPACE / 2.) / MZ_SPACE))
    return float(np.nextafter(edge(i), np.inf))


# ------------------------------------------------------------------ the cases
def golden_clusters():
    """The clusters of tests/golden/cosine_medoid.npz: n = 1..9 and three more, ~30 peaks each."""
    csr = make_clusters_np(0, seed=7, n_template=30, sizes=np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 5, 3, 7]))
    return from_csr(csr)


def _spec(rng, template, jitter=0.002, keep=0.9, lo=None):
    mz = template[rng.random(len(template)) < keep]
    if len(mz) == 0:
        mz = template[:1]
    mz = np.round(np.sort(mz + rng.normal(0, jitter, len(mz))), 5)
    return mz, np.round(rng.lognormal(5, 1.5, len(mz)), 2)


def _cluster(rng, n, n_template, lo=100.0, hi=400.0):
    t = np.sort(rng.uniform(lo, hi, n_template))
    return [_spec(rng, t) for _ in range(n)]


def _grid_spec(rng, pool, k):
    """k peaks on a 0.01 grid (each in a bin of its own: k runs), sorted."""
    mz = np.sort(rng.choice(pool, k, replace=False))
    return mz, np.round(rng.lognormal(5, 1.0, k), 2)


def case_small():
    rng = np.random.default_rng(11)
    a, b, c = _cluster(rng, 3, 20)
    zero = (a[0].copy(), np.zeros(len(a[0])))
    zero2 = (b[0].copy(), np.zeros(len(b[0])))
    return [[a], [a, b], [a, b, c], [zero, b], [zero, zero2, zero]]


def case_duplicates():
    rng = np.random.default_rng(12)
    t = np.sort(rng.uniform(100, 400, 25))
    a = _spec(rng, t, keep=1.0)           # the full template: the most similar to every other member
    b, c, d = (_spec(rng, t, keep=0.6) for _ in range(3))
    dup = lambda s: (s[0].copy(), s[1].copy())  # noqa: E731
    return [[a, b, c, dup(a), d, dup(a)], [b, a, c, d, dup(a)]]


def case_cut():
    rng = np.random.default_rng(13)
    four = _cluster(rng, 4, 15, 100.0, 480.0)  # one template; two members reach ~500, two ~1,500
    lo = [(np.append(m, 500.0 + k), np.append(i, 50.0)) for k, (m, i) in enumerate(four[:2])]
    hi = [(np.append(m, [900.0, 1500.0 + k]), np.append(i, [20.0 + k, 50.0])) for k, (m, i) in enumerate(four[2:])]
    one = [(np.array([200.0]), np.array([5.0])), (np.array([200.001]), np.array([7.0])), (np.array([300.0]), np.array([1.0]))]
    x = ulp_above_edge(250.0)
    alone = [(np.array([100.0, 180.0, x]), np.array([1.0, 2.0, 3.0]))]
    both = [(np.array([100.0, 180.0, x]), np.array([1.0, 2.0, 3.0])), (np.array([100.001, 181.0, x]), np.array([2.0, 1.0, 5.0])),
            (np.array([100.0, 180.0, 240.0]), np.array([1.0, 2.0, 3.0]))]
    mixed = [(np.array([150.0, x]), np.array([1.0, 4.0])), (np.array([150.0, x - 0.004, 260.0]), np.array([2.0, 3.0, 1.0])),
             (np.array([150.001, 249.0]), np.array([1.0, 1.0]))]
    return [[lo[0], hi[0], lo[1], hi[1]], one, one[:1], alone, both, mixed]


def case_order():
    rng = np.random.default_rng(14)
    cl = _cluster(rng, 4, 30)
    p = rng.permutation(len(cl[1][0]))
    while p[-1] == len(p) - 1:  # the last element is not the maximum
        p = rng.permutation(len(p))
    cl[1] = (cl[1][0][p], cl[1][1][p])
    dense = []
    base = np.sort(rng.uniform(100, 300, 12))
    for _ in range(3):  # several peaks per bin, in input order
        mz = np.concatenate([base + rng.normal(0, 0.0006, 12) for _ in range(4)])
        mz = np.round(mz[rng.permutation(len(mz))], 5)
        dense.append((np.append(mz, 310.0), np.round(rng.lognormal(5, 1, len(mz) + 1), 2)))
    bad = [(np.array([-5.0, 120.0, np.nan, 200.0, 0.0, 250.0]), np.array([9.0, 1.0, 9.0, 2.0, 4.0, 3.0])),
           (np.array([120.001, -0.001, 200.0, 249.0]), np.array([2.0, 5.0, 1.0, 1.0])),
           (np.array([np.nan, 0.001, 120.0, 260.0]), np.array([1.0, 3.0, 2.0, 6.0]))]
    return [cl, dense, bad]


def case_empty():
    rng = np.random.default_rng(15)
    a, b, c = _cluster(rng, 3, 10)
    e = (np.zeros(0), np.zeros(0))
    return [[e, a, b], [a, b], [a, e, b], [], [a, b, e], [c], [e]]


def case_run_seams():
    rng = np.random.default_rng(16)
    pool = 100.0 + 0.01 * np.arange(2000)
    return [[_grid_spec(rng, pool[:200], k) for _ in range(3)] for k in (63, 64, 65)]


def case_member_seams():
    rng = np.random.default_rng(17)
    pool = 100.0 + 0.01 * np.arange(60)
    return [[_grid_spec(rng, pool, 8) for _ in range(n)] for n in (LDS_MEMBERS, LDS_MEMBERS + 1, 130)]


def case_lds_runs():
    """LDS_RUNS runs in one cluster and one more in the next."""
    rng = np.random.default_rng(18)
    pool = 100.0 + 0.01 * np.arange(3000)
    at = [_grid_spec(rng, pool, 1024) for _ in range(LDS_RUNS // 1024)]
    past = [_grid_spec(rng, pool, 1024) for _ in range(LDS_RUNS // 1024 - 1)] + [_grid_spec(rng, pool, 1025)]
    assert sum(len(m) for m, _ in at) == LDS_RUNS and sum(len(m) for m, _ in past) == LDS_RUNS + 1
    return [at, past]


def case_long_spectrum():
    rng = np.random.default_rng(19)
    mz = np.round(np.sort(rng.uniform(100, 2000, 5000)), 5)
    big = (mz, np.round(rng.lognormal(5, 1.5, 5000), 2))
    others = []
    for _ in range(2):
        sub = np.sort(rng.choice(5000, 50, replace=False))
        others.append((np.round(mz[sub] + rng.normal(0, 0.002, 50), 5), np.round(rng.lognormal(5, 1.5, 50), 2)))
    return [[others[0], big, others[1]]]


def fuzz_case(seed):
    """Small random batches: n <= 40, <= 120 peaks, the shapes of tests/test_gpu_fuzz.py."""
    rng = np.random.default_rng(5000 + seed)
    C = int(rng.integers(2, 6))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        sizes = rng.integers(1, 13, C)
    elif kind == 1:
        sizes = np.minimum(40, (2 * rng.random(C) ** (-1 / 1.1)).astype(np.int64) + 1)
    else:
        sizes = np.concatenate([rng.integers(25, 41, 1), rng.integers(1, 6, C - 1)])
    n_template = int(rng.choice([1, 5, 30, 60, 100]))
    clusters = [_cluster(rng, int(n), n_template) for n in sizes]
    coarse, unsorted, zeros, empties = rng.random(4) < (0.4, 0.3, 0.2, 0.3)
    out = []
    for cl in clusters:
        new = []
        for mz, it in cl:
            if coarse:  # duplicate bins and exact m/z ties
                mz = np.round(mz, 2)
            if unsorted and rng.random() < 0.2:
                p = rng.permutation(len(mz))
                mz, it = mz[p], it[p]
            if zeros and rng.random() < 0.1:
                it = it.copy()
                it[rng.integers(0, len(it))] = 0.0
            if empties and rng.random() < 0.05:
                mz, it = np.zeros(0), np.zeros(0)
            new.append((mz, it))
        out.append(new)
    if rng.random() < 0.3:
        out.insert(int(rng.integers(0, len(out) + 1)), [])
    return out


N_FUZZ = 20
CASES = {
    "golden": golden_clusters, "small": case_small, "duplicates": case_duplicates, "cut": case_cut,
    "order": case_order, "empty": case_empty, "run_seams": case_run_seams, "member_seams": case_member_seams,
    "lds_runs": case_lds_runs, "long_spectrum": case_long_spectrum,
}
CASES.update({f"fuzz{k}": (lambda k=k: fuzz_case(k)) for k in range(N_FUZZ)})

_cache = {}


def clusters_of(name):
    if name not in _cache:
        cl = CASES[name]()
        _cache[name] = (cl, oracle(cl))
    return _cache[name][0]


def expect(name):
    clusters_of(name)
    return _cache[name][1]
