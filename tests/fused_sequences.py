"""Batches for the fused pass's persistent loop (bin_mean_medoid_kernel walks many clusters
per workgroup; csrc/fused.hip): what one cluster leaves behind meets the next one.

Plain builders (numpy only, no GPU), made of the pieces and constants of
tests/fused_cases.py.  A *kind* is one cluster built to take one of the kernel's paths;
``sequence()`` strings the kinds together so that every ordered pair of kinds -- a kind
followed by itself included -- is adjacent somewhere, which is the order ONE workgroup
walks them in when the grid is capped at 1 (SPX_FU_GRID=1).
tests/test_fused_sequences_inputs.py asserts on the host that every kind has the property
it is named for; tests/test_gpu_fused_persistent.py runs the batches through the kernel.
"""
import numpy as np

import fused_cases as fc

TOL = 0.1


def _raw_spec(mz, rng, prec=500.0, charge=2):
    """A spectrum whose m/z need not be sorted or finite (fc._spec insists on both)."""
    mz = np.asarray(mz, np.float64)
    return {"m/z array": mz, "intensity array": np.round(rng.lognormal(4.0, 1.0, len(mz)), 3),
            "precursor mz": prec, "precursor charge": charge}


# ------------------------------------------------------------------ the kinds
def n2(rng):
    """An ordinary cluster of 2 spectra."""
    return fc._ordinary(rng, 2, 40)


def n50_full(rng):
    """50 spectra whose union holds 1,530 bin-mean bins (BM_DCAP = 1,536) and 1,720 medoid
    columns (64 * MD_KWMAX = 1,728; 27 row words): the LDS at its fullest in both bodies.
    Template peak k sits alone in its 0.02 bin and in its 0.1 bin; the last 190 lie past the
    bin-mean range (they count for the medoid only).  Spectrum s owns the peaks k = s mod 50
    and shares a few of its neighbour's, so the distances differ."""
    inside = np.round(100.05 + 1.2 * np.arange(1530), 5)
    outside = np.round(2000.05 + 0.1 * np.arange(190), 5)
    template = np.concatenate([inside, outside])
    own = [np.arange(s, len(template), 50) for s in range(50)]
    out = []
    for s in range(50):
        ks = np.union1d(own[s], own[(s + 1) % 50][:2 * (s % 5 + 1)])
        out.append(fc._spec(template[ks], rng, 612.3456))
    return out


def n1(rng):
    """A single spectrum: the medoid is that spectrum, no distances."""
    return fc._ordinary(rng, 1, 40)


def n51(rng):
    """51 spectra, one more than BR_NMAX: kNotHere before anything is read."""
    return fc._ordinary(rng, fc.BR_NMAX + 1, 20)


def len253(rng):
    """One spectrum of 253 peaks, one more than BM_FASTLEN: kNotHere at the length vote."""
    step = 1790.0 / 260
    template = np.round(110.0 + step * np.arange(260) + rng.uniform(0.5, step - 0.5, 260), 5)
    return [fc._spec(m, rng) for m in fc._subset_spectra(rng, template, [fc.BM_FASTLEN + 1, 63, 126])]


def mixed_charge(rng):
    """Spectrum 2 has another precursor charge: kMixedCharge, nothing emitted."""
    cl = fc._ordinary(rng, 4, 40)
    cl[2]["precursor charge"] = 3
    return cl


def inversion(rng):
    """Spectrum 1 has one pair of neighbours in descending order, in different bins: the
    register path's vote after phase A defers the cluster (kDeferred)."""
    cl = fc._ordinary(rng, 5, 60, keep=1.0)
    mz = cl[1]["m/z array"].copy()
    mz[20], mz[21] = mz[21], mz[20]
    cl[1] = _raw_spec(mz, rng, cl[0]["precursor mz"])
    return cl


def nan_mz(rng):
    """One NaN m/z in spectrum 0: deferred at the same vote."""
    cl = fc._ordinary(rng, 4, 50, keep=1.0)
    mz = cl[0]["m/z array"].copy()
    mz[17] = np.nan
    cl[0] = _raw_spec(mz, rng, cl[0]["precursor mz"])
    return cl


def d_over(rng):
    """1,537 distinct bin-mean bins, one more than BM_DCAP: kDeferred after phase B."""
    return fc._d_cluster(rng, fc.BM_DCAP + 1)


def k_over(rng):
    """1,729 medoid columns, one more than 64 * MD_KWMAX: the medoid hands the cluster on
    (rep = -4) after the bin-mean completed it."""
    return fc._k_cluster(rng, fc.MD_KMAX + 1)


def md_out(rng):
    """A peak whose ceil(mz / 0.1) is 32,768, the first bin past the register bitmap: the
    bin-mean completes, the medoid runs medoid_small_body inside the fused kernel."""
    cl = fc._ordinary(rng, 4, 50)
    mz_out = float(np.round((fc.MD_BINS - 0.5) * TOL, 5))
    cl[1] = fc._spec(np.concatenate([cl[1]["m/z array"], [mz_out]]), rng, cl[0]["precursor mz"])
    return cl


def all_out(rng):
    """Every peak outside [100, 2000): no bin is occupied, nothing is emitted, the medoid
    still has its columns."""
    below = np.sort(np.round(rng.uniform(50.0, 99.0, 15), 5))
    above = np.sort(np.round(rng.uniform(2001.0, 2600.0, 40), 5))
    out = []
    for _ in range(4):
        kb, ka = rng.random(15) < 0.8, rng.random(40) < 0.8
        out.append(fc._spec(np.concatenate([below[kb], above[ka]]), rng))
    return out


KINDS = {"n2": n2, "n50_full": n50_full, "n1": n1, "n51": n51, "len253": len253, "mixed_charge": mixed_charge,
         "inversion": inversion, "nan_mz": nan_mz, "d_over": d_over, "k_over": k_over, "md_out": md_out,
         "all_out": all_out}
_KIND = {}


def kind(name):
    """The cluster of a kind (a list of spectrum dicts), built once: treat as read-only."""
    if name not in _KIND:
        _KIND[name] = KINDS[name](np.random.default_rng(200 + list(KINDS).index(name)))
    return _KIND[name]


def kind_csr(name):
    return fc._pack([kind(name)])


# ------------------------------------------------------------------ the sequence
def pair_walk(k):
    """A closed walk over 0..k-1 in which every ordered pair (a, b), a == b included, is
    adjacent exactly once: an Euler circuit of the complete digraph with loops (Hierholzer),
    k * k + 1 vertices long."""
    nxt = [list(range(k - 1, -1, -1)) for _ in range(k)]  # unused edges a -> nxt[a].pop()
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


_SEQ = []


def sequence():
    """(csr, names): one batch of len(KINDS)^2 + 1 clusters, names[c] the kind of cluster c,
    every ordered pair of kinds adjacent.  Built once (treat as read-only)."""
    if not _SEQ:
        names = [list(KINDS)[i] for i in pair_walk(len(KINDS))]
        _SEQ.append((fc._pack([kind(n) for n in names]), names))
    return _SEQ[0]


def ordinary_batch(n_clusters, seed=300):
    """n_clusters small ordinary clusters (2-6 spectra of ~30 peaks): the grid-edge batches."""
    rng = np.random.default_rng(seed)
    return fc._pack([fc._ordinary(rng, int(rng.integers(2, 7)), 30) for _ in range(n_clusters)])
