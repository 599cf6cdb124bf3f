"""Inputs for the register tail past 32 spectra, one Gram tile per wave, and for the diagonal
tiles' shared operand fragment (medoid_tail_regs, specpride_amd/csrc/medoid.hip).

Plain builders (numpy only, no GPU) in the manner of tests/medoid_tail_cases.py, whose
palette and helpers they reuse: each returns ``(SpectraCSR, facts)``.
tests/test_medoid_p4_inputs.py proves on the host that every case has the property it is
named for; tests/test_gpu_medoid_p4.py runs them through the kernels.  medoid_tail_cases'
``sizes`` and ``row_words`` cover the leaf and tile edges at one row word; the cases here are
the ones the four-wave tail adds: the hand-off at every kind of row-tile-1 work and every
row-word count, sums that expose a reordered addition, the argmin across the two finishing
waves, empty spectra around the tile edge, a stale hand-off in a persistent workgroup, and
operands that differ between a diagonal tile's rows and an off-diagonal tile's.
"""
import numpy as np

import fused_cases as fc
import medoid_tail_cases as tc
from fused_cases import MD_KMAX, _pack, _spec
from medoid_tail_cases import TOL, _k_cluster, _tiny
from oracle import np_oracle

# row tile 1 holds: only the sequential tail (33, 39), no tail (40, 48), strided groups and
# a tail (41, 47, 49, 50); past the fused register path the same again (57 / 56, 64 / 63)
FUSED_SIZES = (33, 39, 40, 41, 47, 48, 49, 50)
OVER_SIZES = (56, 57, 63, 64)
ROW_WORDS = {1: 40, 3: 130, 27: MD_KMAX}  # KW -> K distinct medoid bins
SEED_BUDGET = 64


def distances(csr, c, tol=TOL):
    """The full symmetric matrix d[i, j] = 1 - xcorr(i, j) of cluster c, as the reference
    forms each entry (most_similar_representative.py:13-19)."""
    spectra = [m for (m, _i) in csr.cluster(c)]
    n = len(spectra)
    d = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            d[i, j] = d[j, i] = 1.0 - np_oracle.xcorr(spectra[i], spectra[j], tol)
    return d


def handoff(kw, ns=FUSED_SIZES, seed=401):
    """One cluster per size of exactly ROW_WORDS[kw] distinct medoid bins.
    facts: n (cluster -> size), K, KW."""
    rng = np.random.default_rng(seed + kw)
    K = ROW_WORDS[kw]
    clusters = [_k_cluster(rng, K, n) for n in ns]
    return _pack(clusters), dict(n={c: n for c, n in enumerate(ns)}, K=K, KW=kw)


def _reorder_sensitive(d):
    """Columns j of d whose total changes when each accumulator takes row tile 1's terms
    before row tile 0's, and those where a row or column sum does."""
    import medoid_p4_model as pm

    n = d.shape[0]
    sums, tots = [], []
    for j in range(n):
        a, b = pm.chain_sums(d, j, (0, 1)), pm.chain_sums(d, j, (1, 0))
        if a != b:
            sums.append(j)
        if (a[0] + a[1]) / np.float64(n) != (b[0] + b[1]) / np.float64(n):
            tots.append(j)
    return sums, tots


def reordered(ns=(41, 50), seed=410):
    """Per size the first seeded candidate (tiny spectra of 3..12 palette peaks) in which some
    spectrum's TOTAL changes in its last bits when row tile 1's terms are added before row
    tile 0's; fails if the seed budget holds none.  facts: n, seed, columns (cluster ->
    the columns whose total changes)."""
    clusters, facts = [], dict(n={}, seed={}, columns={})
    for n in ns:
        for k in range(SEED_BUDGET):
            rng = np.random.default_rng(seed + 1000 * n + k)
            cl = _tiny(rng, n, lo=3)
            _, tots = _reorder_sensitive(distances(_pack([cl]), 0))
            if tots:
                c = len(clusters)
                facts["n"][c], facts["seed"][c], facts["columns"][c] = n, k, tots
                clusters.append(cl)
                break
        else:
            raise AssertionError(f"no order-sensitive cluster of {n} spectra within {SEED_BUDGET} seeds")
    return _pack(clusters), facts


def _minima(rng, n, where):
    """The spectra `where` hold the same 12 bins S; every other spectrum holds 6 bins of S
    and 6 of its own: d = 1/2 to each of `where`, more among each other on average."""
    S = np.arange(12)
    cl = []
    for s in range(n):
        ks = S if s in where else np.concatenate([rng.choice(S, 6, replace=False), 12 + 6 * s + np.arange(6)])
        cl.append(_spec(np.round(200.05 + 0.1 * np.sort(ks), 5), rng))
    return cl


def argmin_waves(seed=420):
    """The minimum total only in a column >= 32; equal minima in a column < 32 and one
    >= 32; the minimum in column 32 itself -- at n = 40 and 50.
    facts: where (cluster -> the spectra that hold the minimum)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(where={}, n={})
    for n in (40, 50):
        for where in ((36,), (5, 36), (32,)):
            facts["where"][len(clusters)] = where
            facts["n"][len(clusters)] = n
            clusters.append(_minima(rng, n, where))
    return _pack(clusters), facts


def empties_past_32(seed=430):
    """An empty spectrum at index 0, 31, 32 and n - 1 of a cluster of 50 (one each, and all
    four), and a cluster of 40 whose every spectrum holds two peaks in one medoid bin.
    facts: empty (cluster -> indices), shared (the cluster of 40)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(empty={})
    for where in ((0,), (31,), (32,), (49,), (0, 31, 32, 49)):
        cl = _tiny(rng, 50, lo=1)
        for j in where:
            cl[j] = _spec(np.zeros(0), rng)
        facts["empty"][len(clusters)] = where
        clusters.append(cl)
    cl = []
    for _ in range(40):
        ks = np.sort(rng.choice(tc.PALETTE, int(rng.integers(2, 12)), replace=False))
        mz = 200.05 + 0.1 * ks
        cl.append(_spec(np.round(np.sort(np.concatenate([mz, mz[:1] + 0.021])), 5), rng))
    facts["shared"] = len(clusters)
    clusters.append(cl)
    return _pack(clusters), facts


STALE_SIZES = (50, 8, 33, 2, 50, 32, 41)


def stale_handoff(seed=440):
    """What one workgroup walks in this order: n = 50, 8, 33, 2, 50, 32, 41 -- a hand-off
    written, then clusters that write none, then one that must not read the old one -- with
    two clusters that leave the fused register path at run time (fused_cases.deferrals: a
    medoid bin past the table) between them; nine clusters, an odd total, so the two header
    buffers change roles from one walk to the next.
    facts: sizes (cluster -> n for the register-path clusters), early (the two others)."""
    rng = np.random.default_rng(seed)
    dcsr, _ = fc.deferrals(n_clusters=2, seed=7)
    early = [[{"m/z array": np.array(m), "intensity array": np.array(i), "precursor mz": 500.0,
               "precursor charge": 2} for (m, i) in dcsr.cluster(c)] for c in range(2)]
    clusters, facts = [], dict(sizes={}, early=[])
    for k, n in enumerate(STALE_SIZES):
        if k in (3, 5):
            facts["early"].append(len(clusters))
            clusters.append(early.pop())
        facts["sizes"][len(clusters)] = n
        clusters.append(_tiny(rng, n, lo=1))
    return _pack(clusters), facts


def diagonal(seed=450):
    """n = 2, 17, 32 at KW = 1 (K = 64) and 27 (K = 1,728).  In column order (the rank of a
    bin in the cluster's union) the odd spectra hold content in the first 32 columns only or
    in the last 32 only, alternately; the even ones also carry the columns between, shared
    out among them, so the union is exactly K (at n = 2 both spectra do, and are longer than
    the fused register path takes).  Rows that differ this much from the columns they meet
    change a count if an operand is shared off the diagonal, or not shared on it.
    facts: n, KW, K (cluster -> value), narrow (cluster -> {spectrum: 'first' | 'last'})."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(n={}, KW={}, K={}, narrow={})
    for kw, K in ((1, 64), (27, MD_KMAX)):
        first, last, middle = np.arange(0, 32), np.arange(K - 32, K), np.arange(32, K - 32)
        for n in (2, 17, 32):
            fillers = [s for s in range(n) if s % 2 == 0 or n == 2]
            cl, narrow = [], {}
            for s in range(n):
                if s in fillers:
                    f = fillers.index(s)
                    ks = set(middle[f::len(fillers)].tolist())
                    if n == 2:  # the two halves of the union, four columns in common
                        ks |= set(first.tolist()) if f == 0 else set(last.tolist()) | set(first[:4].tolist())
                    elif f == 0:
                        ks |= set(first.tolist()) | set(last.tolist())
                    else:
                        ks |= set(rng.choice(first, 4, replace=False).tolist())
                        ks |= set(rng.choice(last, 4, replace=False).tolist())
                else:
                    narrow[s] = "first" if s % 4 == 1 else "last"
                    pool = first if narrow[s] == "first" else last
                    ks = set(rng.choice(pool, int(rng.integers(3, 12)), replace=False).tolist())
                cl.append(_spec(np.round(1900.05 + 0.1 * np.array(sorted(ks)), 5), rng))
            c = len(clusters)
            facts["n"][c], facts["KW"][c], facts["K"][c], facts["narrow"][c] = n, kw, K, narrow
            clusters.append(cl)
    return _pack(clusters), facts


# name -> (builder, through the fused pass too, every cluster completes in its register bodies)
CASES = {
    "handoff_kw1": (lambda: handoff(1), True, True),
    "handoff_kw3": (lambda: handoff(3), True, True),
    "handoff_kw27": (lambda: handoff(27), True, True),
    "handoff_over_kw1": (lambda: handoff(1, OVER_SIZES, seed=402), False, False),
    "handoff_over_kw3": (lambda: handoff(3, OVER_SIZES, seed=402), False, False),
    "handoff_over_kw27": (lambda: handoff(27, OVER_SIZES, seed=402), False, False),
    "reordered": (reordered, True, True),
    "argmin_waves": (argmin_waves, True, True),
    "empties_past_32": (empties_past_32, True, True),
    "stale_handoff": (stale_handoff, True, False),
    "diagonal": (diagonal, True, False),
}

_built = {}


def case(name):
    """(csr, facts, fused, clean) of a case, built once and shared (callers leave it unchanged)."""
    if name not in _built:
        builder, fused, clean = CASES[name]
        csr, facts = builder()
        _built[name] = (csr, facts, fused, clean)
    return _built[name]
