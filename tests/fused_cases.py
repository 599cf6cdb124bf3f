"""Inputs for the fused bin-mean + medoid pass (spx_bin_mean_medoid) at its own edges.

Plain builders (numpy only, no GPU): each returns ``(SpectraCSR, facts)`` where
``facts`` names the clusters built to have a property.  tests/test_fused_inputs.py
asserts on the host that every case HAS the property it is named for;
tests/test_gpu_fused.py runs them through the kernel.  Every spectrum is m/z-sorted
(an unsorted one leaves the register path, which is not what these cases are about).

The kernel constants the cases are built around.  Retune one, update this table:

    BR_NMAX     50     specpride_amd/csrc/bin_mean.hip:474  spectra per cluster of the register path
    BM_FASTLEN  252    specpride_amd/csrc/bin_mean.hip:73   peaks per spectrum (4 waves x 63 owner lanes)
    BM_WMAX     1536   specpride_amd/csrc/bin_mean.hip:74   64-bit words of the bin-mean bin space
    BM_DCAP     1536   specpride_amd/csrc/bin_mean.hip:75   distinct occupied bin-mean bins per cluster
    MD_KWMAX    27     specpride_amd/csrc/medoid.hip:35     row words: 64 * 27 = 1,728 medoid columns
    MD_BINS     32768  specpride_amd/csrc/bin_mean.hip:514  32 * BR_MDW32 medoid bins ceil(mz/tol)
"""
import numpy as np

from oracle import np_oracle
from specpride_amd.csr import SpectraCSR

BR_NMAX = 50
BM_FASTLEN = 252
BM_WMAX = 1536
BM_DCAP = 1536
MD_KWMAX = 27
MD_KMAX = 64 * MD_KWMAX
MD_BINS = 32768
WAVE_PEAKS = 63  # owner lanes per wave: the seams sit between peaks 62/63, 125/126, 188/189
SEAMS = (62, 125, 188)

DEFAULT_BIN = dict(minimum=100.0, maximum=2000.0, binsize=0.02, apply_peak_quorum=True)
NARROW_BIN = dict(minimum=300.0, maximum=1200.0, binsize=0.05)
WIDE_BIN = dict(minimum=100.0, maximum=2000.0, binsize=0.005)


# ------------------------------------------------------------------ host facts
def bin_kw(**kw):
    p = dict(DEFAULT_BIN)
    p.update(kw)
    return p


def n_words(**kw):
    """64-bit words of the bin space (spx_api.hip bin_words; binning.py:172)."""
    p = bin_kw(**kw)
    return (int((p["maximum"] - p["minimum"]) / p["binsize"]) + 1 + 63) // 64


def in_range(mz, **kw):
    p = bin_kw(**kw)
    mz = np.asarray(mz, np.float64)
    return (mz >= p["minimum"]) & (mz < p["maximum"])


def bin_mean_bins(mz, **kw):
    """The bin indices np_oracle.bin_mean_cluster gives the in-range peaks (binning.py:190)."""
    p = bin_kw(**kw)
    mz = np.asarray(mz, np.float64)
    return ((mz[in_range(mz, **kw)] - p["minimum"]) / p["binsize"]).astype(np.int64)


def cluster_mz(csr, c):
    return csr.mz[csr.spec_off[csr.cluster_off[c]]:csr.spec_off[csr.cluster_off[c + 1]]]


def cluster_D(csr, c, **kw):
    """Distinct occupied bin-mean bins of cluster c."""
    return len(np.unique(bin_mean_bins(cluster_mz(csr, c), **kw)))


def cluster_K(csr, c, tol=0.1):
    """Distinct medoid bins ceil(mz/tol) over the cluster's union (its column count)."""
    return len(np_oracle.xcorr_bins(cluster_mz(csr, c), tol))


def spectrum_lengths(csr, c):
    s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
    return np.diff(csr.spec_off[s0:s1 + 1])


def clipped(csr, **kw):
    """The batch with every peak outside [minimum, maximum) dropped."""
    keep = in_range(csr.mz, **kw)
    spec_of = np.repeat(np.arange(csr.n_spectra), np.diff(csr.spec_off))
    lens = np.bincount(spec_of[keep], minlength=csr.n_spectra)
    spec_off = np.zeros(csr.n_spectra + 1, np.int64)
    np.cumsum(lens, out=spec_off[1:])
    return SpectraCSR(csr.cluster_off, spec_off, csr.mz[keep], csr.inten[keep], csr.prec_mz, csr.charge, csr.rt)


def fits_register_path(csr, c, tol=0.1, **kw):
    """Whether both register bodies of the fused kernel complete cluster c (nothing
    handed on): the caps of the table above, on m/z-sorted finite single-charge spectra."""
    n = int(csr.cluster_off[c + 1] - csr.cluster_off[c])
    mz = cluster_mz(csr, c)
    if n < 1 or len(mz) == 0:
        return False
    bins = np_oracle.xcorr_bins(mz, tol)
    return (n <= BR_NMAX and n_words(**kw) <= BM_WMAX and spectrum_lengths(csr, c).max() <= BM_FASTLEN
            and cluster_D(csr, c, **kw) <= BM_DCAP and bins.min() >= 0 and bins.max() < MD_BINS
            and (n == 1 or ((len(bins) + 63) // 64 | 1) <= MD_KWMAX))


# ------------------------------------------------------------------ pieces
def _spec(mz, rng, prec=500.0, charge=2):
    mz = np.asarray(mz, np.float64)
    assert np.all(np.diff(mz) >= 0)
    return {"m/z array": mz, "intensity array": np.round(rng.lognormal(4.0, 1.0, len(mz)), 3),
            "precursor mz": prec, "precursor charge": charge}


def _ordinary(rng, n, npk, lo=120.0, hi=1900.0, keep=0.9):
    """n noisy copies of one template of npk peaks in [lo, hi): an everyday cluster."""
    base = np.sort(rng.uniform(lo, hi, npk))
    prec = float(np.round(rng.uniform(400, 900), 4))
    out = []
    for _ in range(n):
        k = rng.random(npk) < keep
        mz = np.sort(np.round(base[k] + rng.normal(0.0, 0.003, int(k.sum())), 5))
        out.append(_spec(mz, rng, prec))
    return out


def _subset_spectra(rng, template, lengths):
    """One spectrum per length: a random subset of the template (jittered), sorted."""
    out = []
    for L in lengths:
        pick = np.sort(rng.choice(len(template), L, replace=False))
        out.append(np.sort(np.round(template[pick] + rng.normal(0.0, 0.002, L), 5)))
    return out


def _pack(clusters):
    return SpectraCSR.from_clusters(clusters)


# ------------------------------------------------------------------ out_of_range
def out_of_range(minimum=100.0, maximum=2000.0, seed=101):
    """Peaks on both sides of [minimum, maximum) and exactly on its ends, m/z in [50, 2600].

    facts: edges (a cluster holding minimum, maximum and nextafter(maximum, 0) exactly),
    spectrum_out (cluster, spectrum: one spectrum wholly out of range), cluster_out (a
    cluster wholly out of range: D = 0), flip (a cluster whose medoid changes when the
    out-of-range peaks are dropped)."""
    rng = np.random.default_rng(seed)
    lo_all, hi_all = 50.0, 2600.0
    below = lambda k: np.round(rng.uniform(lo_all, minimum - 0.5, k), 5)  # noqa: E731
    above = lambda k: np.round(rng.uniform(maximum + 0.5, hi_all, k), 5)  # noqa: E731
    clusters = [_ordinary(rng, 5, 80, lo_all, hi_all)]
    # the ends themselves, in every spectrum, among peaks on both sides
    ends = np.array([minimum, np.nextafter(maximum, 0.0), maximum])
    base = np.sort(rng.uniform(lo_all, hi_all, 60))
    edges = []
    for _ in range(6):
        k = rng.random(60) < 0.85
        edges.append(_spec(np.sort(np.concatenate([np.round(base[k] + rng.normal(0, 0.003, int(k.sum())), 5), ends])),
                           rng))
    clusters.append(edges)
    clusters.append(_ordinary(rng, 2, 40, lo_all, hi_all))
    # one spectrum wholly out of range (it still counts in the quorum's n and in the medoid)
    part = _ordinary(rng, 8, 90, minimum + 1.0, maximum - 1.0)
    outside = np.sort(np.concatenate([below(30), above(50)]))
    part[3] = _spec(outside, rng, part[0]["precursor mz"])
    # the others share some of its out-of-range peaks: the medoid sees them
    for j in (0, 5):
        part[j] = _spec(np.sort(np.concatenate([part[j]["m/z array"], outside[::3]])), rng, part[0]["precursor mz"])
    clusters.append(part)
    clusters.append(_ordinary(rng, 12, 120, lo_all, hi_all))
    # a cluster wholly out of range: the bin-mean emits nothing
    tb, ta = np.sort(below(20)), np.sort(above(60))
    allout = []
    for _ in range(4):
        kb, ka = rng.random(20) < 0.8, rng.random(60) < 0.8
        allout.append(_spec(np.concatenate([tb[kb], ta[ka]]), rng))
    clusters.append(allout)
    # the medoid must keep what the bin-mean drops: in range spectrum 0 holds every peak of
    # the others (clipped: xcorr 1 with each, the medoid); out of range the others agree
    # with each other and spectrum 0 with nobody (full: the medoid is one of the others)
    step = (maximum - minimum - 10.0) / 20.0
    t_in = np.round(minimum + 5.0 + step * np.arange(20) + 0.03, 5)
    t_out = np.round(maximum + 5.0 + 0.5 * np.arange(60) + 0.03, 5)
    flip = [_spec(np.concatenate([t_in, t_out + 0.25]), rng)]
    for s in range(3):
        sub = np.sort(rng.choice(20, 10, replace=False))
        flip.append(_spec(np.concatenate([t_in[sub], t_out]), rng))
    clusters.append(flip)
    clusters.append(_ordinary(rng, 3, 60, lo_all, hi_all))
    return _pack(clusters), dict(edges=1, spectrum_out=(3, 3), cluster_out=5, flip=6, ends=ends)


# ------------------------------------------------------------------ lengths
LENGTHS = (0, 1, 62, 63, 64, 125, 126, 127, 189, 251, 252, 253)


def lengths(with_253=True, seed=102):
    """Spectra of exactly the LENGTHS, in clusters of 3 and 4 spectra.

    facts: lengths (cluster -> spectrum lengths), seam_same / seam_diff (seam peak i ->
    (cluster, spectra): peaks i and i + 1 of those spectra share their bin-mean bin and
    their medoid bin / share neither), long (the cluster with the 253-peak spectrum)."""
    rng = np.random.default_rng(seed)
    plan = [[62, 63, 0], [64, 1, 125, 126], [127, 189, 251], [252, 0, 1, 64]]
    seam_plan = {62: [64, 126, 63], 125: [127, 189, 62], 188: [251, 252, 1, 125]}
    clusters, facts = [], dict(lengths={}, seam_same={}, seam_diff={}, long=None)

    def template():
        step = 1790.0 / 260
        return np.round(110.0 + step * np.arange(260) + rng.uniform(0.5, step - 0.5, 260), 5)

    def add(lens, seam=None):
        mzs = _subset_spectra(rng, template(), lens)
        if seam is not None:
            for s in (0, 1):  # peak seam at x.x41, peak seam + 1 at x.x47: one 0.02 bin, one 0.1 bin
                mzs[s][seam] = np.round(np.floor(mzs[s][seam] * 10.0) / 10.0 + 0.041, 5)
                mzs[s][seam + 1] = np.round(mzs[s][seam] + 0.006, 5)
        c = len(clusters)
        clusters.append([_spec(m, rng) for m in mzs])
        facts["lengths"][c] = list(lens)
        return c

    clusters.append(_ordinary(rng, 4, 90))
    for lens in plan[:2]:
        add(lens)
    for i in SEAMS:
        facts["seam_same"][i] = (add(seam_plan[i], seam=i), (0, 1))
        facts["seam_diff"][i] = (add(seam_plan[i]), (0, 1))
    clusters.append(_ordinary(rng, 3, 200))
    for lens in plan[2:]:
        add(lens)
    if with_253:
        facts["long"] = add([253, 63, 126])
    clusters.append(_ordinary(rng, 2, 30))
    return _pack(clusters), facts


# ------------------------------------------------------------------ counts
def counts(with_51=True, seed=103):
    """Clusters of 1, 2, 3, 49, 50 and 51 spectra of ~30 peaks; one of 50 whose last
    spectrum is empty, one of 3 whose middle one is.

    facts: sizes (cluster -> n), empty_last, empty_middle, over (the 51-spectrum cluster)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [], dict(sizes={}, over=None)

    def add(n, empty=()):
        cl = _ordinary(rng, n, 30)
        for j in empty:
            cl[j] = _spec(np.zeros(0), rng, cl[0]["precursor mz"])
        facts["sizes"][len(clusters)] = n
        clusters.append(cl)
        return len(clusters) - 1

    clusters.append(_ordinary(rng, 4, 60))
    for n in (1, 2, 3, 49):
        add(n)
    clusters.append(_ordinary(rng, 7, 60))
    add(50)
    facts["empty_last"] = add(50, empty=(49,))
    facts["empty_middle"] = add(3, empty=(1,))
    if with_51:
        facts["over"] = add(51)
    clusters.append(_ordinary(rng, 5, 60))
    return _pack(clusters), facts


# ------------------------------------------------------------------ k_columns
def _k_cluster(rng, K):
    """8 spectra whose union is exactly K medoid bins (tol 0.1): bin k at m/z
    1900.05 + 0.1 k, owned by spectrum k % 8; spectrum s also holds the first 2 (s + 1)
    bins of spectrum s + 1, so the distances differ.  Only the bins below m/z 2,000 (at
    most 1,000) are in the default bin-mean range: D stays under BM_DCAP."""
    own = [[k for k in range(K) if k % 8 == s] for s in range(8)]
    out = []
    for s in range(8):
        ks = sorted(set(own[s]) | set(own[(s + 1) % 8][:2 * (s + 1)]))
        out.append(_spec(np.round(1900.05 + 0.1 * np.array(ks), 5), rng))
    return out


def k_columns(Ks=(64, 65, 1728, 1729), seed=104):
    """One cluster each with exactly K distinct ceil(mz/0.1) bins.  facts: K (cluster -> K)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [_ordinary(rng, 5, 100)], dict(K={})
    for K in Ks:
        facts["K"][len(clusters)] = K
        clusters.append(_k_cluster(rng, K))
        clusters.append(_ordinary(rng, 3, 70))
    return _pack(clusters), facts


# ------------------------------------------------------------------ d_bins
def _d_cluster(rng, D):
    """8 spectra whose union is exactly D bin-mean bins at the default parameters: bin b
    at its centre 100.01 + 0.02 b; bins 0..15 common (spectrum s holds the first 16 - s % 4:
    they pass the quorum), bin 16 + 8 i + s owned by spectrum s."""
    own = {s: [16 + 8 * i + s for i in range((D - 16 - s + 7) // 8)] for s in range(8)}
    own = {s: [b for b in bs if b < D] for s, bs in own.items()}
    out = []
    for s in range(8):
        bs = np.array(sorted(set(range(16 - s % 4)) | set(own[s])))
        out.append(_spec(np.round(100.01 + 0.02 * bs, 5), rng))
    return out


def d_bins(Ds=(1536, 1537), seed=105):
    """One cluster each with exactly D distinct bin-mean bins.  facts: D (cluster -> D)."""
    rng = np.random.default_rng(seed)
    clusters, facts = [_ordinary(rng, 6, 100)], dict(D={})
    for D in Ds:
        facts["D"][len(clusters)] = D
        clusters.append(_d_cluster(rng, D))
        clusters.append(_ordinary(rng, 3, 70))
    return _pack(clusters), facts


# ------------------------------------------------------------------ medoid_range
def medoid_range(tol=0.1, seed=106):
    """Peaks whose ceil(mz/tol) is MD_BINS - 1 (the last bin of the register bitmap) and
    MD_BINS (the first one past it), and a peak at m/z 0.0.

    facts: last_in (a cluster reaching bin 32767 and no further; one spectrum starts with
    m/z 0.0), first_out (spectrum 0 starts with m/z 0.0 = the cluster's lowest bin, spectrum
    1 holds bin 32768 and not bin 0), both (bin 32768 in two spectra that also share the
    cluster's lowest bin), mz_in / mz_out (the two m/z)."""
    rng = np.random.default_rng(seed)
    mz_in = float(np.round((MD_BINS - 1.5) * tol, 5))
    mz_out = float(np.round((MD_BINS - 0.5) * tol, 5))
    hi = mz_in - 10 * tol
    lo = min(120.0, hi / 4)

    def cluster(n, npk, tails, heads=None):
        base = np.sort(rng.uniform(lo, hi, npk))
        out = []
        for s in range(n):
            k = rng.random(npk) < 0.9
            mz = np.round(base[k] + rng.normal(0.0, tol / 40, int(k.sum())), 5)
            mz = np.sort(mz[mz < hi])
            mz = np.concatenate([(heads or {}).get(s, []), mz, tails.get(s, [])])
            out.append(_spec(mz, rng))
        return out

    clusters = [_ordinary(rng, 4, 60, lo, hi)]
    clusters.append(cluster(4, 80, {1: [mz_in], 2: [mz_in]}, {2: [0.0]}))
    clusters.append(_ordinary(rng, 3, 60, lo, hi))
    clusters.append(cluster(4, 80, {1: [mz_out]}, {0: [0.0]}))
    clusters.append(cluster(5, 80, {0: [mz_in, mz_out], 3: [mz_out], 4: [mz_in]}, {0: [1.5 * tol], 3: [1.5 * tol]}))
    clusters.append(_ordinary(rng, 6, 60, lo, hi))
    return _pack(clusters), dict(last_in=1, first_out=3, both=4, mz_in=mz_in, mz_out=mz_out)


# ------------------------------------------------------------------ ceil_ties
def ceil_ties(seed=107):
    """m/z that are exact decimal multiples of the tolerances (round(k * 0.1, 5),
    round(k * 0.05, 5)): the quotient mz/tol sits on or next to an integer, which the
    reciprocal product cannot decide.  Several peaks per medoid bin within a spectrum,
    exact m/z ties across spectra, and clusters whose best total is shared.

    facts: ties (cluster -> the spectra sharing the minimal total, at every tolerance)."""
    rng = np.random.default_rng(seed)

    def grid(n, npk, unit, lo_k, hi_k, runs=True):
        ks = np.sort(rng.choice(np.arange(lo_k, hi_k), npk, replace=False))
        if runs:  # runs k, k + 1, k + 2: neighbours in one medoid bin
            ks = np.unique(np.concatenate([ks, ks[::5] + 1, ks[::7] + 2]))
        out = []
        for _ in range(n):
            k = rng.random(len(ks)) < 0.85
            out.append(_spec(np.round(ks[k] * unit, 5), rng))
        return out

    clusters = [grid(6, 80, 0.05, 2000, 32000)]
    clusters.append(grid(5, 100, 0.1, 1000, 16000))
    facts = dict(ties={})
    a = np.round(np.arange(3000, 3040, 4) * 0.1, 5)  # 10 peaks, distinct bins at every tolerance here
    b = np.concatenate([a[:5], np.round(a[5:] + 1.0, 5)])
    facts["ties"][len(clusters)] = (0, 1)
    clusters.append([_spec(a, rng), _spec(b, rng)])                      # n = 2: total0 == total1
    clusters.append(grid(12, 150, 0.05, 2000, 32000))
    facts["ties"][len(clusters)] = (0, 1, 2, 3)
    clusters.append([_spec(a, rng) for _ in range(4)])                   # identical: every total 0
    facts["ties"][len(clusters)] = (0, 2)
    dense = np.round(np.arange(8000, 8060) * 0.05, 5)                    # several peaks per bin
    half = np.concatenate([dense[:30], np.round(dense[30:] + 10.0, 5)])
    clusters.append([_spec(dense, rng), _spec(half, rng), _spec(dense, rng)])        # X, Y, X: total0 == total2
    clusters.append(grid(3, 60, 0.1, 1000, 16000, runs=False))
    return _pack(clusters), facts


# ------------------------------------------------------------------ wide_params
def wide_params(seed=108):
    """An ordinary batch; called with WIDE_BIN its bin space is past BM_WMAX words, so the
    bin-mean register path takes no cluster (kNotHere) and every medoid runs
    medoid_small_body inside the fused kernel."""
    rng = np.random.default_rng(seed)
    clusters = [_ordinary(rng, n, npk) for n, npk in ((1, 40), (2, 60), (7, 100), (20, 150), (3, 30), (12, 80))]
    return _pack(clusters), dict()


# ------------------------------------------------------------------ deferrals
def deferrals(n_clusters=40, seed=7):
    """The recipe of test_medoid_many_runtime_deferrals: small clusters (2-23 spectra) with
    m/z up to 4,500, past the 32,768-bin table at tolerance 0.1: deferred at run time."""
    rng = np.random.default_rng(seed)
    clusters = []
    for _c in range(n_clusters):
        n = int(rng.integers(2, 24))
        base = np.sort(rng.uniform(100.0, 4500.0, 150))
        spectra = []
        for _s in range(n):
            keep = rng.random(150) > 0.1
            mz = np.sort(np.round(base[keep] + rng.normal(0.0, 0.003, int(keep.sum())), 5))
            spectra.append(_spec(mz, rng))
        clusters.append(spectra)
    return _pack(clusters), dict()


# ------------------------------------------------------------------ registry
# name -> (builder, its arguments, [(bin-mean keywords, medoid tolerance), ...]): the
# parameters each case is run with, by the host checks and by the GPU tests alike
CASES = {
    "out_of_range": (out_of_range, (), [(dict(), 0.1)]),
    "out_of_range_narrow": (out_of_range, (300.0, 1200.0), [(dict(NARROW_BIN, apply_peak_quorum=True), 0.1),
                                                           (dict(NARROW_BIN, apply_peak_quorum=False), 0.1)]),
    "lengths": (lengths, (), [(dict(), 0.1)]),
    "counts": (counts, (), [(dict(), 0.1)]),
    "k_columns": (k_columns, (), [(dict(), 0.1)]),
    "d_bins": (d_bins, (), [(dict(), 0.1)]),
    "medoid_range_0.1": (medoid_range, (0.1,), [(dict(), 0.1)]),
    "medoid_range_0.02": (medoid_range, (0.02,), [(dict(), 0.02)]),
    "ceil_ties": (ceil_ties, (), [(dict(), 0.1), (dict(), 0.05), (dict(), 0.3)]),
    "wide_params": (wide_params, (), [(dict(WIDE_BIN), 0.1)]),
    "deferrals": (deferrals, (), [(dict(), 0.1)]),
}
_BUILT = {}


def case(name):
    """(csr, facts) of a registered case, built once (treat as read-only)."""
    if name not in _BUILT:
        builder, args, _ = CASES[name]
        _BUILT[name] = builder(*args)
    return _BUILT[name]


def runs(name):
    return CASES[name][2]
