"""Inputs for the medoid's register tail (medoid_tail_regs, specpride_amd/csrc/medoid.hip):
the Gram tiles, the lane-pair sums and the argmin at the leaf and tile edges.

Plain builders (numpy only, no GPU), in the manner of tests/fused_cases.py: each returns
``(SpectraCSR, facts)``.  tests/test_medoid_tail_inputs.py proves on the host, against the
oracle, that every case has the property it is named for; tests/test_gpu_medoid_tail.py
runs them through the kernels.  Spectra hold 0..12 peaks drawn from a palette of 40 medoid
bins, so the batches are tiny and equal distances and totals are common; only the row-word
cases need more bins than that and use ~36 peaks per spectrum.

Kernel constants the cases are built around (retune one, update this table):

    SPX_MD_MFMA_NMIN  1   csrc/medoid.hip   the register tail for n above it: every cluster
    MD_NMAX           64  csrc/medoid.hip   spectra per cluster of the small kernels
    BR_NMAX           50  csrc/bin_mean.hip spectra per cluster of the fused register path
    MD_KWMAX          27  csrc/medoid.hip   row words: 64 * 27 = 1,728 medoid columns
"""
import numpy as np

from fused_cases import MD_KMAX, _pack, _spec

NMIN = 1  # SPX_MD_MFMA_NMIN: clusters of n = NMIN and NMIN + 1 are in every size list
# the leaf (multiples of 8) and tile (32) edges, and BR_NMAX
FUSED_SIZES = (NMIN, NMIN + 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 39, 40, 41, 47, 48, 49, 50)
OVER_SIZES = (51, 63, 64, 65)  # 51: past the fused register path; 65: past the small kernels
TOL = 0.1
PALETTE = 40


def _mz_of_bins(ks, rng):
    """One peak inside medoid bin ceil(mz / 0.1) = 2001 + k for each k (sorted)."""
    ks = np.sort(np.asarray(ks, np.int64))
    return np.round(200.05 + 0.1 * ks + rng.uniform(-0.02, 0.02, len(ks)), 5)


def _tiny(rng, n, lo=0, hi=12):
    """n spectra of lo..hi peaks, each a random subset of the palette."""
    out = []
    for _ in range(n):
        k = int(rng.integers(lo, hi + 1))
        out.append(_spec(_mz_of_bins(rng.choice(PALETTE, k, replace=False), rng), rng))
    return out


def sizes(ns=FUSED_SIZES, seed=301):
    """One cluster per size, tiny spectra of 1..12 peaks.  facts: n (cluster -> size)."""
    rng = np.random.default_rng(seed)
    clusters = [_tiny(rng, n, lo=1) for n in ns]
    return _pack(clusters), dict(n={c: n for c, n in enumerate(ns)})


def _k_cluster(rng, K, n):
    """n spectra whose union is exactly K medoid bins: bin k belongs to spectrum k % n, and
    spectrum s also holds the first s % 5 bins of spectrum s + 1.  m/z from 1900.05 up, so at
    most 1,000 bins lie inside the default bin-mean range."""
    own = [[k for k in range(K) if k % n == s] for s in range(n)]
    out = []
    for s in range(n):
        ks = sorted(set(own[s]) | set(own[(s + 1) % n][:s % 5]))
        out.append(_spec(np.round(1900.05 + 0.1 * np.array(ks), 5), rng))
    return out


def row_words(Ks=(40, 64, 65, MD_KMAX - 1, MD_KMAX), ns=(12, 40), seed=302):
    """Clusters of exactly K distinct medoid bins: KW = 1 (K <= 64), 3, and 27 (K <= 1,728).
    facts: K (cluster -> K)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(K={})
    for K in Ks:
        for n in ns:
            facts["K"][len(clusters)] = K
            clusters.append(_k_cluster(rng, K, n))
    return _pack(clusters), facts


def row_words_over(seed=303):
    """K = 1,729 and 1,800: more row words than the register bodies hold, handed on."""
    return row_words(Ks=(MD_KMAX + 1, 1800), seed=seed)


def empties(seed=304):
    """An empty spectrum first, in the middle and last, at n = 9, 33 and 50; and all three.
    facts: empty (cluster -> local indices of the empty spectra)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(empty={})
    for n in (9, 33, 50):
        for where in ((0,), (n // 2,), (n - 1,), (0, n // 2, n - 1)):
            cl = _tiny(rng, n, lo=1)
            for j in where:
                cl[j] = _spec(np.zeros(0), rng)
            facts["empty"][len(clusters)] = where
            clusters.append(cl)
    return _pack(clusters), facts


def identical(seed=305):
    """Every spectrum of a cluster the same 7 bins: every total equal, representative 0."""
    rng = np.random.default_rng(seed)
    clusters = []
    for n in (2, 8, 33, 50):
        ks = rng.choice(PALETTE, 7, replace=False)
        clusters.append([_spec(_mz_of_bins(ks, rng), rng) for _ in range(n)])
    return _pack(clusters), dict(n=(2, 8, 33, 50))


def two_minima(lo=5, hi=40, n=50, seed=306):
    """Spectra lo and hi hold the same 12 bins S; every other spectrum holds 6 bins of S and 6
    of its own: d = 1/2 to lo and hi, more among each other on average.  The minimum total
    is attained at lo and hi only -- one in each column wave."""
    rng = np.random.default_rng(seed)
    S = np.arange(12)
    cl = []
    for s in range(n):
        if s in (lo, hi):
            ks = S
        else:
            ks = np.concatenate([rng.choice(S, 6, replace=False), 12 + 6 * s + np.arange(6)])
        cl.append(_spec(np.round(200.05 + 0.1 * np.sort(ks), 5), rng))
    return _pack([_tiny(rng, 4, lo=1), cl, _tiny(rng, 3, lo=1)]), dict(cluster=1, lo=lo, hi=hi)


def shared_bin(seed=307):
    """Every spectrum holds two peaks inside one medoid bin: |B_i| < p_i, so d(i, i) > 0.
    Clusters of 9 and 40 spectra."""
    rng = np.random.default_rng(seed)
    clusters = []
    for n in (9, 40):
        cl = []
        for _ in range(n):
            ks = np.sort(rng.choice(PALETTE, int(rng.integers(2, 12)), replace=False))
            mz = 200.05 + 0.1 * ks
            mz = np.sort(np.concatenate([mz, mz[:1] + 0.021]))  # a second peak in the first bin
            cl.append(_spec(np.round(mz, 5), rng))
        clusters.append(cl)
    return _pack(clusters), dict(n=(9, 40))


# name -> (builder, whether the fused pass completes every cluster in its register bodies)
CASES = {
    "sizes": (sizes, True),
    "sizes_over": (lambda: sizes(OVER_SIZES, seed=308), False),
    "row_words": (row_words, True),
    "row_words_over": (row_words_over, False),
    "empties": (empties, True),
    "identical": (identical, True),
    "two_minima": (two_minima, True),
    "shared_bin": (shared_bin, True),
}

_built = {}


def case(name):
    """(csr, facts, clean) of a case, built once and shared (callers leave it unchanged)."""
    if name not in _built:
        csr, facts = CASES[name][0]()
        _built[name] = (csr, facts, CASES[name][1])
    return _built[name]
