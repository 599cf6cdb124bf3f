"""Inputs for the fused pass's step bodies after their instruction diet (bin_mean.hip
phases A-C, fused.hip medoid_from_codes): lanes that issue no LDS atomic, m/z on the edges
of the two reciprocal-product bands, equal bins across the wave seams, codes whose two
halves carry their largest values, and one sequence of all of them for a small grid.

Plain builders (numpy only, no GPU), each ``(SpectraCSR, facts)``.
tests/test_fused_diet_inputs.py proves the named properties on the host with the
kernel's own arithmetic restated in float64; tests/test_gpu_fused_diet.py runs the
batches through the kernel.  Every batch has at most 8 clusters.
"""
import numpy as np

import fused_cases as fc
import fused_sequences as fs

TOL = 0.1
BM_BAND = 2.0 ** -30   # trunc_div_small (spx_device.hpp): q - trunc(q) outside (b, 1 - b) divides
MD_BAND = 2.0 ** -24   # kDivBand: ceil(q) - q outside (b, 1 - b) divides
NO_QUORUM = dict(apply_peak_quorum=False)

# the classes of a reciprocal-product fraction f against a band b; the first five take
# the division, the last two the fast path next to it
DIV_CLASSES = ("zero", "in_lo", "in_hi", "last_in_lo", "last_in_hi")
FAST_CLASSES = ("first_out_lo", "first_out_hi")
CLASSES = DIV_CLASSES + FAST_CLASSES


# ------------------------------------------------------------------ the kernel's fractions
def bm_fraction(mz, minimum=100.0, binsize=0.02):
    """(q, f) of phase A's bin-mean bin: q = (m - minimum) * (1 / binsize), f = q - trunc(q)."""
    x = np.asarray(mz, np.float64) - minimum
    q = x * (1.0 / binsize)
    return q, q - np.trunc(q)


def md_fraction(mz, tol=TOL):
    """(q, f) of phase A's medoid bin: q = m * (1 / tol), f = ceil(q) - q."""
    q = np.asarray(mz, np.float64) * (1.0 / tol)
    return q, np.ceil(q) - q


def classify(q, f, band):
    """Class name per element ('' where f is well inside the fast range).  The fractions
    are multiples of ulp(q): 'last inside' is f == b (or 1 - b) exactly, 'first outside'
    the two representable fractions next to it on the fast side."""
    q, f = np.asarray(q), np.asarray(f)
    u = np.spacing(np.abs(q))
    out = np.full(f.shape, "", dtype=object)
    out[(f > band) & (f <= band + 2 * u)] = "first_out_lo"
    out[(f < 1.0 - band) & (f >= 1.0 - band - 2 * u)] = "first_out_hi"
    out[(f > 0.0) & (f < band)] = "in_lo"
    out[(f > 1.0 - band) & (f < 1.0)] = "in_hi"
    out[f == band] = "last_in_lo"
    out[f == 1.0 - band] = "last_in_hi"
    out[f == 0.0] = "zero"
    return out


def _neighbours(x, half):
    """The doubles within `half` ulps of x > 0, ascending."""
    bits = np.float64(x).view(np.int64) + np.arange(-half, half + 1, dtype=np.int64)
    return bits.view(np.float64)


def _search(points, fraction, band, half):
    """class -> [m/z]: for every grid point, the double nearest to it in each class."""
    found = {c: [] for c in CLASSES}
    for p in points:
        cand = _neighbours(p, half)
        cls = classify(*fraction(cand), band)
        mid = len(cand) // 2
        for c in CLASSES:
            idx = np.flatnonzero(cls == c)
            if len(idx):
                found[c].append(float(cand[idx[np.argmin(np.abs(idx - mid))]]))
    return found


# ------------------------------------------------------------------ band_edges
BM_POINTS = (37, 1001, 40213, 77777, 94001)   # bins k: m/z 100 + 0.02 k
MD_POINTS = (1203, 5557, 9999, 14142, 18888)  # bins k: m/z 0.1 k


def _band_cluster(rng):
    """(cluster, bm, md): see band_edges."""
    bm = _search([100.0 + 0.02 * k for k in BM_POINTS], bm_fraction, BM_BAND, 4096)
    md = _search([TOL * k for k in MD_POINTS], md_fraction, MD_BAND, 1 << 18)
    spectra = [[], [], [], []]
    for k in BM_POINTS:
        spectra[2].append(100.0 + 0.02 * (k - 0.5))
        spectra[3].append(100.0 + 0.02 * (k + 0.5))
    for c in CLASSES:
        for m in bm[c]:
            spectra[0].append(m)
            spectra[1].append(m)
    for k in MD_POINTS:
        spectra[1].append(TOL * (k - 0.5))
        spectra[2].append(TOL * (k + 0.5))
    for c in CLASSES:
        spectra[0].extend(md[c])
    filler = np.round(np.sort(rng.uniform(150.0, 1850.0, 40)), 5)
    cluster = []
    for special in spectra:
        keep = rng.random(40) < 0.9
        cluster.append(fc._spec(np.sort(np.concatenate([filler[keep], special])), rng))
    return cluster, bm, md


def band_edges(seed=401):
    """Four spectra that hold, for both bin functions, m/z whose fraction falls in every
    class of CLASSES around several grid points.  A bin-mean special sits in spectra 0 and
    1; spectrum 2 holds the centre of the bin below the grid point and spectrum 3 the
    centre of the one above, so a peak binned on the wrong side changes a mean.  A medoid
    special sits in spectrum 0, with the centres of the bins on both sides in spectra 1
    and 2, so a wrong side changes a distance.  Run without the quorum: every bin is emitted.

    facts: bm / md (class -> [m/z])."""
    rng = np.random.default_rng(seed)
    cluster, bm, md = _band_cluster(rng)
    return fc._pack([fc._ordinary(rng, 3, 50), cluster, fc._ordinary(rng, 5, 70)]), dict(cluster=1, bm=bm, md=md)


# ------------------------------------------------------------------ idle_lanes
IDLE_LENGTHS = (1, 62, 63, 64, 126, 127, 189, 190, 252)


def _idle_cluster(rng):
    step = 1790.0 / 260
    template = np.round(110.0 + step * np.arange(260) + rng.uniform(0.5, step - 0.5, 260), 5)
    cl = [fc._spec(m, rng) for m in fc._subset_spectra(rng, template, IDLE_LENGTHS)]
    # 40 doubles inside bin-mean bin [700.04, 700.06) and medoid bin (700.0, 700.1]
    one = np.sort(np.round(700.041 + 0.0004 * np.arange(40), 5))
    cl.append(fc._spec(one, rng))
    return cl


def idle_lanes(seed=402):
    """One cluster with spectra of the IDLE_LENGTHS (whole waves, or all lanes of a wave
    but one, with no peak) and one spectrum of 40 peaks that all share one bin-mean bin
    and one medoid bin (one valid lane; same-address ORs for the medoid); and a cluster
    with every peak outside [100, 2000): D = 0, no lane ever has a bin-mean contribution.

    facts: lengths (the cluster), one_bin (its spectrum), all_out (the cluster)."""
    rng = np.random.default_rng(seed)
    cl = _idle_cluster(rng)
    return (fc._pack([fc._ordinary(rng, 4, 60), cl, fs.all_out(rng), fc._ordinary(rng, 2, 30)]),
            dict(lengths=1, one_bin=len(IDLE_LENGTHS), all_out=2))


# ------------------------------------------------------------------ seams
def _seam_cluster(rng, share):
    step = 1790.0 / 260
    template = np.round(110.0 + step * np.arange(260) + rng.uniform(0.5, step - 0.5, 260), 5)
    mzs = fc._subset_spectra(rng, template, [252, 252, 252])
    if share:
        for m in mzs:
            for i in fc.SEAMS:  # x.x41 and x.x47: one 0.02 bin, one 0.1 bin
                m[i] = np.round(np.floor(m[i] * 10.0) / 10.0 + 0.041, 5)
                m[i + 1] = np.round(m[i] + 0.006, 5)
    return [fc._spec(m, rng) for m in mzs]


def seams(seed=403):
    """Two clusters of three 252-peak spectra.  In `same`, peaks i and i + 1 share their
    bin-mean bin and their medoid bin at every wave seam i = 62, 125, 188 (peak i is then
    not the last of its bin: lane 62 learns it from lane 63's key); in `diff` no
    neighbours share a bin.  facts: same, diff (clusters)."""
    rng = np.random.default_rng(seed)
    return (fc._pack([_seam_cluster(rng, True), fc._ordinary(rng, 3, 40), _seam_cluster(rng, False)]),
            dict(same=0, diff=2))


# ------------------------------------------------------------------ packing
PACK_SIZES = (1, 2, 3, 49, 50)


def _full_cluster(rng, n):
    """n spectra whose codes carry the largest values n allows.  n >= 49: the union holds
    1,530 bin-mean bins and 1,720 medoid columns (fused_sequences.n50_full's template, dealt
    to n spectra).  n <= 3: every spectrum has 252 peaks, each alone in its bins (252 n
    slots and columns, all a cluster of n spectra can hold)."""
    if n >= 49:
        inside = np.round(100.05 + 1.2 * np.arange(1530), 5)
        outside = np.round(2000.05 + 0.1 * np.arange(190), 5)
        template = np.concatenate([inside, outside])
        own = [np.arange(s, len(template), n) for s in range(n)]
        return [fc._spec(template[np.union1d(own[s], own[(s + 1) % n][:2 * (s % 5 + 1)])], rng, 612.3456)
                for s in range(n)]
    template = np.round(100.05 + 2.4 * np.arange(252 * n), 5)
    return [fc._spec(template[s::n], rng, 498.7654) for s in range(n)]


def packing(sizes=PACK_SIZES, seed=404):
    """One full cluster (see _full_cluster) per size.  Odd n leaves the last spectrum's
    code unpaired in phase C.  facts: sizes (cluster -> n)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(sizes={})
    for n in sizes:
        facts["sizes"][len(clusters)] = n
        clusters.append(_full_cluster(rng, n))
    clusters.append(fc._ordinary(rng, 4, 50))
    return fc._pack(clusters), facts


# ------------------------------------------------------------------ sequence
def sequence(seed=405):
    """The kinds above in one batch, with a kNotHere cluster (51 spectra) and a
    mixed-charge cluster between them: under a grid of 1 or 2 workgroups each follows an
    early exit of another kind.  facts: kinds (cluster -> name)."""
    rng = np.random.default_rng(seed)
    band = _band_cluster(rng)[0]
    idle = _idle_cluster(rng)
    seam = _seam_cluster(rng, True)
    kinds = [("full49", _full_cluster(rng, 49)), ("not_here", fs.n51(rng)), ("band", band),
             ("mixed_charge", fs.mixed_charge(rng)), ("idle", idle), ("all_out", fs.all_out(rng)),
             ("seam", seam), ("full3", _full_cluster(rng, 3))]
    return fc._pack([c for _, c in kinds]), dict(kinds={i: k for i, (k, _) in enumerate(kinds)})


_BUILT = {}


def case(name):
    """(csr, facts) of a builder above, built once (treat as read-only)."""
    if name not in _BUILT:
        _BUILT[name] = globals()[name]()
    return _BUILT[name]
