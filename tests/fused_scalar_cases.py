"""Inputs for the fused pass after its set-up and scalar-stream changes (bin_mean.hip
bin_mean_reg_path_t, fused.hip medoid_from_codes): phase A's first ring loads go out ahead
of the set-up's LDS work, and the band edges of the two reciprocal products live in scalar
registers for the cluster.  What can go wrong there: a wave's lanes at a spectrum's end, a
ring deeper than the cluster, a return taken with the ring's loads in flight, one
workgroup walking from cluster to cluster, and constants that outlive their call.

Plain builders (numpy only, no GPU), each ``(SpectraCSR, facts)``, made of the pieces of
tests/fused_cases.py, tests/fused_sequences.py and tests/fused_diet_cases.py.
tests/test_fused_scalar_inputs.py proves the named properties on the host;
tests/test_gpu_fused_scalar.py runs the batches through the kernel.
"""
import numpy as np

import fused_cases as fc
import fused_diet_cases as dc
import fused_sequences as fs

TOL = 0.1
PFA = 6  # SPX_BR_PFA_MD (bin_mean.hip): the fused pass's phase-A ring depth

# every wave's boundary of 63 owned lanes, one below and one above
EDGE_LENGTHS = (1, 62, 63, 64, 125, 126, 127, 188, 189, 190, 251, 252)
RING_SIZES = (1, 2, 5, 6, 7, 12, 13, 50, 51)
# the kinds of tests/fused_sequences.py that return before the medoid's stepped path, by
# what the kernel does with them
EARLY_KINDS = ("mixed_charge", "inversion", "nan_mz", "d_over", "md_out", "n1")


def _template(rng):
    step = 1790.0 / 260
    return np.round(110.0 + step * np.arange(260) + rng.uniform(0.5, step - 0.5, 260), 5)


def _of_lengths(rng, lengths):
    """One cluster with a spectrum of each length, subsets of one template."""
    return [fc._spec(m, rng) for m in fc._subset_spectra(rng, _template(rng), lengths)]


# ------------------------------------------------------------------ mask_edges
def mask_edges(seed=501):
    """Each EDGE_LENGTH alone (a cluster of two spectra of that length) and all of them in
    one cluster; clusters with a zero-length spectrum first, in the middle and last.

    facts: alone (length -> cluster), mixed (cluster), empty (position -> cluster)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(alone={}, mixed=None, empty={})
    for L in EDGE_LENGTHS:
        facts["alone"][L] = len(clusters)
        clusters.append(_of_lengths(rng, [L, L]))
    facts["mixed"] = len(clusters)
    clusters.append(_of_lengths(rng, list(rng.permutation(EDGE_LENGTHS))))
    for name, lens in (("first", [0, 64, 126]), ("middle", [63, 0, 190]), ("last", [127, 62, 0])):
        facts["empty"][name] = len(clusters)
        clusters.append(_of_lengths(rng, lens))
    return fc._pack(clusters), facts


# ------------------------------------------------------------------ ring_depths
def ring_depths(seed=502):
    """Clusters of RING_SIZES spectra (the ring holds PFA = 6: fewer spectra than slots,
    exactly as many, one more, two rings' worth and one more; 50 completes the register
    path, 51 is handed on), and a 253-peak spectrum (kNotHere at the length vote) followed
    by an ordinary cluster.

    facts: sizes (cluster -> n), long (the cluster with the 253-peak spectrum)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(sizes={}, long=None)
    for n in RING_SIZES:
        facts["sizes"][len(clusters)] = n
        clusters.append(fc._ordinary(rng, n, 40))
    facts["long"] = len(clusters)
    clusters.append(fs.len253(rng))
    clusters.append(fc._ordinary(rng, 4, 60))
    return fc._pack(clusters), facts


# ------------------------------------------------------------------ early_returns
def early_returns(kind):
    """The kind first, in the middle and last in a batch of five, ordinary clusters between.
    facts: at (the kind's clusters), between (the ordinary ones)."""
    rng = np.random.default_rng(510 + EARLY_KINDS.index(kind))
    k = fs.kind(kind)
    clusters = [k, fc._ordinary(rng, 7, 80), k, fc._ordinary(rng, 13, 50), k]
    return fc._pack(clusters), dict(at=(0, 2, 4), between=(1, 3))


# ------------------------------------------------------------------ walks
def walk(n_clusters=40, seed=520):
    """Ordinary clusters of 2..14 spectra (below, at and above the ring's depth) for one
    workgroup to walk: every cluster completes both register bodies, so each one's first
    loads are issued right after its predecessor's medoid."""
    rng = np.random.default_rng(seed)
    return fc._pack([fc._ordinary(rng, int(rng.integers(2, 15)), 40) for _ in range(n_clusters)]), dict()


def walk_ends_off_path(last="md_out", seed=521):
    """Six ordinary clusters and a last one that leaves the stepped path (its header is the
    last the loop fetches; nothing follows it)."""
    rng = np.random.default_rng(seed)
    clusters = [fc._ordinary(rng, int(rng.integers(2, 15)), 40) for _ in range(6)] + [fs.kind(last)]
    return fc._pack(clusters), dict(last=6)


def few(n_clusters, seed=522):
    """0, 1 or 2 ordinary clusters."""
    rng = np.random.default_rng(seed)
    return fc._pack([fc._ordinary(rng, 5, 40) for _ in range(n_clusters)]), dict()


# ------------------------------------------------------------------ band_constants
PARAMS_A = dict(minimum=100.0, maximum=2000.0, binsize=0.02)
PARAMS_B = dict(minimum=300.0, maximum=1200.0, binsize=0.05)
TOL_A, TOL_B = 0.1, 0.2
B_POINTS = (41, 1001, 7777, 17999)  # bins k of PARAMS_B: m/z 300 + 0.05 k


def band_constants(seed=530):
    """One cluster of four spectra holding, for BOTH parameter sets: a peak exactly at the
    minimum, the double just below it, the double just below the maximum and the maximum
    itself; m/z on bin edges of both grids whose reciprocal-product fraction lies in the
    band (they take the division); and, for PARAMS_A and TOL_A, every band class of
    tests/fused_diet_cases.py.  An ordinary cluster on either side.

    facts: cluster, ends (params name -> the four m/z), edges (params name -> [m/z] on bin
    edges that divide)."""
    rng = np.random.default_rng(seed)
    band, _, _ = dc._band_cluster(rng)
    ends, edges = {}, {}
    for name, p, pts in (("A", PARAMS_A, dc.BM_POINTS), ("B", PARAMS_B, B_POINTS)):
        lo, hi = p["minimum"], p["maximum"]
        ends[name] = [float(np.nextafter(lo, 0.0)), lo, float(np.nextafter(hi, 0.0)), hi]
        found = dc._search([lo + p["binsize"] * k for k in pts],
                           lambda m, lo=lo, w=p["binsize"]: dc.bm_fraction(m, lo, w), dc.BM_BAND, 4096)
        edges[name] = sorted(set(found["zero"] + found["in_lo"] + found["in_hi"]))
    extra = np.array(sorted(set(ends["A"] + ends["B"] + edges["A"] + edges["B"])))
    cluster = []
    for s, sp in enumerate(band):
        mz = sp["m/z array"]
        if s < 2:  # the ends and the edges in two spectra: their bins pass a quorum of 2
            mz = np.sort(np.concatenate([mz, extra]))
        cluster.append(fc._spec(mz, rng))
    return (fc._pack([fc._ordinary(rng, 3, 50, 50.0, 2400.0), cluster, fc._ordinary(rng, 5, 70, 50.0, 2400.0)]),
            dict(cluster=1, ends=ends, edges=edges))


_BUILT = {}


def case(name, *args):
    """(csr, facts) of a builder above, built once per argument list (treat as read-only)."""
    if (name, args) not in _BUILT:
        _BUILT[(name, args)] = globals()[name](*args)
    return _BUILT[(name, args)]
