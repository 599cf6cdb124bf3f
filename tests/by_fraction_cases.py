"""Explained b/y intensity (benchmark.fraction_of_by, reference src/benchmark.py:40-61):
a numpy restatement of what spectrum_utils and pyteomics do for that function, an
order-free brute-force formulation of the same rules, and the named cases the CPU and
GPU tests share.

Neither library is installed, so the restatement is written from the libraries' documented
behaviour (the issue's rules 1-8; DESIGN.md section 4 gives its standing: parity is
unpinned at that boundary).  ``restate`` follows the libraries' loops literally -- stable
sort by m/z, range mask, precursor mask, the fragment list sorted by m/z, a two-pointer
window walk, ``np.argmax``, sequential sums in peak order -- and shares nothing with the
kernel's formulation (no sort, binary search or full scan under a comparator, a bitmap).

A case is a dict of host arrays shaped like ``engine.by_fraction``'s arguments: ``mz``,
``inten``, ``seg_begin``, ``seg_end``, ``prec_mz``, ``charge``, ``peptides`` (list of str)
and ``params`` (overrides of the defaults, by field name or residue letter)."""
import functools

import numpy as np

RTOL = 1e-12  # two sums of at most 5,000 non-negative terms: n * 2^-53 = 5.6e-13 each way
STATUS_OK, STATUS_UNRESOLVED = 0, 100
MAX_SEQ, MAX_CHARGE = 256, 64  # the engine's limits
N_FUZZ = 4

RESIDUES = "QWERTYIPASDFGHKLCVNM"
AA_MASS = {"G": 57.02146, "A": 71.03711, "S": 87.03203, "P": 97.05276, "V": 99.06841, "T": 101.04768,
           "C": 103.00919, "L": 113.08406, "I": 113.08406, "N": 114.04293, "D": 115.02694, "Q": 128.05858,
           "K": 128.09496, "E": 129.04259, "M": 131.04049, "H": 137.05891, "F": 147.06841, "R": 156.10111,
           "Y": 163.06333, "W": 186.07931}
DEFAULTS = dict(h=1.00782503207, o=15.99491461956, proton=1.00727646677, precursor_proton=1.0072766,
                min_mz=100.0, max_mz=1400.0, tol_ppm=50.0)


def params_of(overrides=None):
    """(aa_mass dict, constants dict) with the overrides applied (a residue letter or a field)."""
    aa, const = dict(AA_MASS), dict(DEFAULTS)
    for k, v in (overrides or {}).items():
        (aa if len(k) == 1 else const)[k] = v
    return aa, const


def fast_mass(seq, ion, q, aa, const):
    """pyteomics mass.fast_mass(seq, ion_type=ion, charge=q) for ion 'b' or 'y'."""
    m = 0.0
    for r in seq:
        m += aa[r]
    m += const["h"] * 2 + const["o"]
    if ion == "b":
        m += (const["h"] * -2) + (const["o"] * -1)
    return (m + const["proton"] * q) / q


def fragments(seq, z, aa, const):
    """The m/z of every b/y fragment annotate_peptide_fragments considers, in its loop order."""
    out = []
    for i in range(1, len(seq)):
        for q in range(1, max(1, z - 1) + 1):
            out.append(fast_mass(seq[:i], "b", q, aa, const))
            out.append(fast_mass(seq[i:], "y", q, aa, const))
    return out


def precursor_mzs(prec_mz, z, const):
    neutral = (prec_mz - const["precursor_proton"]) * z
    return [neutral / c + const["precursor_proton"] for c in range(z, 0, -1)]


def _early(seq, prec_mz, z, mz, aa):
    """(fraction, status) where no spectrum is built, else None."""
    if len(seq) > MAX_SEQ:
        return float("nan"), STATUS_UNRESOLVED
    if any(not (r in aa and aa[r] == aa[r]) for r in seq):
        return 0.0, STATUS_OK
    if z > MAX_CHARGE or not np.isfinite(prec_mz) or not np.all(np.isfinite(mz)):
        return float("nan"), STATUS_UNRESOLVED
    return None


def restate(seq, prec_mz, z, mz, inten, overrides=None, detail=False):
    """(fraction, status) of one spectrum, the libraries' way.  ``detail``: also the kept and
    the annotated peaks as sorted arrays of input indices."""
    aa, const = params_of(overrides)
    mz, inten = np.asarray(mz, np.float64), np.asarray(inten, np.float64)
    none = np.zeros(0, np.int64)
    early = _early(seq, prec_mz, z, mz, aa)
    if early is not None:
        return (*early, none, none) if detail else early
    tol = const["tol_ppm"]
    order = np.argsort(mz, kind="stable")                   # MsmsSpectrum sorts its peaks by m/z
    idx, mz, inten = order, mz[order], inten[order]
    keep = (mz >= const["min_mz"]) & (mz <= const["max_mz"])  # set_mz_range
    idx, mz, inten = idx[keep], mz[keep], inten[keep]
    if z > 0:                                               # remove_precursor_peak, isotope 0
        mask = np.ones(len(mz), bool)
        for r in precursor_mzs(prec_mz, z, const):
            mask &= ~(np.abs((mz - r) / r * 1e6) <= tol)
        idx, mz, inten = idx[mask], mz[mask], inten[mask]
    annotated = np.zeros(len(mz), bool)                     # annotate_peptide_fragments, most_intense
    lo = 0
    for f in sorted(fragments(seq, z, aa, const)):
        while lo < len(mz) and (mz[lo] - f) / f * 1e6 < -tol:
            lo += 1
        hi = lo
        while hi < len(mz) and (mz[hi] - f) / f * 1e6 <= tol:
            hi += 1
        if hi > lo:
            annotated[lo + int(np.argmax(inten[lo:hi]))] = True
    current, by_current = 0., 0.                            # benchmark.py:53-61
    for ix in range(len(inten)):
        current += float(inten[ix])
        if annotated[ix]:
            by_current += float(inten[ix])
    fraction = by_current / current if current > 0. else 0.0
    if detail:
        return fraction, STATUS_OK, np.sort(idx), np.sort(idx[annotated])
    return fraction, STATUS_OK


def brute(seq, prec_mz, z, mz, inten, overrides=None):
    """The same rules with no sort: (kept, annotated) input indices, every fragment against
    every peak under the comparator (intensity descending with NaN first, m/z ascending,
    index ascending).  None where no spectrum is built."""
    aa, const = params_of(overrides)
    mz, inten = np.asarray(mz, np.float64), np.asarray(inten, np.float64)
    if _early(seq, prec_mz, z, mz, aa) is not None:
        return None
    tol = const["tol_ppm"]
    kept = (mz >= const["min_mz"]) & (mz <= const["max_mz"])
    for r in precursor_mzs(prec_mz, z, const) if z > 0 else []:
        kept &= ~(np.abs((mz - r) / r * 1e6) <= tol)
    chosen = set()
    is_nan = np.isnan(inten)
    for f in fragments(seq, z, aa, const):
        x = (mz - f) / f * 1e6
        cand = np.flatnonzero(kept & (x >= -tol) & (x <= tol))
        if len(cand):
            chosen.add(int(min(cand, key=lambda k: (not is_nan[k], 0.0 if is_nan[k] else -inten[k], mz[k], k))))
    return np.flatnonzero(kept), np.array(sorted(chosen), np.int64)


# ------------------------------------------------------------------ building cases
def peptide(rng, n):
    return "".join(rng.choice(list(RESIDUES), size=n))


def precursor_of(seq, z, default=500.0):
    """The peptide's own precursor m/z at charge z (a fixed value for no charge or no residues)."""
    if z <= 0 or not seq:
        return default
    aa, const = params_of()
    return fast_mass(seq, "y", z, aa, const)


def fragment_spectrum(rng, seq, z, n_true=40, n_noise=40, jitter_ppm=15.0, sort=True, overrides=None, total=None):
    """Peaks at up to n_true of the peptide's fragments (jittered, so some leave their window)
    plus uniform noise (``total``: as much noise as makes that many peaks), strictly positive
    intensities."""
    aa, const = params_of(overrides)
    fr = np.array([f for f in fragments(seq, z, aa, const) if 90.0 < f < 1500.0])
    if len(fr) > n_true:
        fr = rng.choice(fr, size=n_true, replace=False)
    if total is not None:
        n_noise = total - len(fr)
    mz = np.concatenate([fr * (1.0 + rng.normal(0.0, jitter_ppm, len(fr)) * 1e-6), rng.uniform(80.0, 1500.0, n_noise)])
    inten = np.round(rng.lognormal(5.0, 1.5, len(mz)), 2) + 0.01
    if sort:
        order = np.argsort(mz, kind="stable")
        mz, inten = mz[order], inten[order]
    else:
        order = rng.permutation(len(mz))
        mz, inten = mz[order], inten[order]
    return mz, inten


def pack(spectra, params=None):
    """A case from spectra given as (peptide, prec_mz, charge, mz, inten): back-to-back segments."""
    off = np.zeros(len(spectra) + 1, np.int64)
    np.cumsum([len(s[3]) for s in spectra], out=off[1:])
    cat = lambda k: (np.concatenate([np.asarray(s[k], np.float64) for s in spectra])  # noqa: E731
                     if spectra else np.zeros(0))
    return dict(mz=cat(3), inten=cat(4), seg_begin=off[:-1].copy(), seg_end=off[1:].copy(),
                prec_mz=np.array([s[1] for s in spectra], np.float64),
                charge=np.array([s[2] for s in spectra], np.int32), peptides=[s[0] for s in spectra],
                params=dict(params or {}))


def _c_lengths_charges():
    rng = np.random.default_rng(101)
    out = []
    for n in (0, 1, 2, 7, 50, 256):
        seq = peptide(rng, n)
        for z in (0, 1, 2, 3, 4, 16):
            out.append((seq, precursor_of(seq, z), z, *fragment_spectrum(rng, seq, z, n_true=120, n_noise=60)))
    return pack(out)


WK = ("WK", 187.08658646677, 147.11280115047)  # the peptide, its b1 and its y1 (charge 2: zmax = 1)


def _c_window():
    """A peak just inside and just outside the 50 ppm window, on both sides, for b1 and y1."""
    out = []
    for f in WK[1:]:
        for ppm in (49.9, 50.1, -49.9, -50.1):
            out.append(("WK", 400.0, 2, [f * (1 + ppm * 1e-6), 300.0], [10.0, 5.0]))
    b1 = WK[1]
    out.append(("WK", 400.0, 2, [b1 * (1 - 50.1e-6), b1 * (1 - 49.9e-6), b1 * (1 + 49.9e-6), b1 * (1 + 50.1e-6)],
                [1.0, 2.0, 4.0, 8.0]))
    return pack(out)


def _c_shared_tied():
    aa, const = params_of()
    g2 = fast_mass("GG", "b", 1, aa, const)  # = b4 of GGGG at charge 2: one peak, two fragments
    seq = "GGGGK"
    y1 = fast_mass("K", "y", 1, aa, const)
    out = [(seq, 600.0, 3, [g2, y1, 700.0], [6.0, 3.0, 1.0]),
           # two peaks in one window, the stronger one second; then equal intensities
           (seq, 600.0, 3, [y1 * (1 - 10e-6), y1 * (1 + 10e-6), 700.0], [5.0, 9.0, 2.0]),
           (seq, 600.0, 3, [y1 * (1 - 10e-6), y1 * (1 + 10e-6), 700.0], [7.0, 7.0, 2.0]),
           # equal m/z and equal intensity: the lower index
           (seq, 600.0, 3, [y1, y1, 700.0], [7.0, 7.0, 2.0])]
    return pack(out)


def _c_tie_union():
    """A's window holds P1 and P2 with equal intensity, B's only P2: the union is {P1, P2}
    because A takes P1 (the lower m/z); the other tie-break would give {P2}.  B = b2 of GAK
    sits 80 ppm above A = y1 through a changed mass of A."""
    aa, const = params_of()
    a = fast_mass("K", "y", 1, aa, const)
    mass_a = a * (1 + 80e-6) - aa["G"] - const["proton"]
    ov = {"A": mass_a}
    aa2, _ = params_of(ov)
    b = fast_mass("GA", "b", 1, aa2, const)
    p1, p2 = a * (1 - 30e-6), a * (1 + 40e-6)
    assert abs((p2 - b) / b * 1e6) < 45 and (p1 - b) / b * 1e6 < -100
    return pack([("GAK", 500.0, 2, [p1, p2, 800.0], [4.0, 4.0, 8.0]),
                 ("GAK", 500.0, 2, [p2, p1, 800.0], [4.0, 4.0, 8.0])], params=ov)


def _c_precursor():
    """prec 300 at charge 3: the precursor at charges 3, 2, 1 is removed; 60 ppm away is kept."""
    _, const = params_of()
    r3, r2, r1 = precursor_mzs(300.0, 3, const)
    seq = "PEPTIDEK"
    aa, _ = params_of()
    y1, b2 = fast_mass("K", "y", 1, aa, const), fast_mass("PE", "b", 1, aa, const)
    mz = [y1, b2, r3, r2, r1, r2 * (1 + 60e-6), r1 * (1 - 49e-6), r3 * (1 + 49e-6), r1 * (1 - 60e-6)]
    inten = [5.0, 7.0, 100.0, 200.0, 400.0, 11.0, 13.0, 17.0, 19.0]
    out = [(seq, 300.0, 3, mz, inten), (seq, 300.0, 1, mz, inten), (seq, 300.0, 0, mz, inten),
           (seq, 300.0, -2, mz, inten), (seq, 300.0, 64, mz, inten)]
    return pack(out)


def _c_range_ends():
    aa, const = params_of()
    y1 = fast_mass("K", "y", 1, aa, const)
    return pack([("PEPTIDEK", 700.0, 2, [99.999, 100.0, y1, 1400.0, 1400.001], [64.0, 1.0, 2.0, 4.0, 128.0]),
                 ("PEPTIDEK", 700.0, 2, [99.999, 1400.001], [64.0, 128.0])])


def _c_empty_zero():
    aa, const = params_of()
    y1 = fast_mass("K", "y", 1, aa, const)
    return pack([("PEPTIDEK", 700.0, 2, [], []), ("PEPTIDEK", 700.0, 2, [y1, 300.0], [0.0, 0.0]),
                 ("", 700.0, 2, [y1, 300.0], [1.0, 2.0]), ("PEPTIDEK", 700.0, 2, [y1, 300.0], [1.0, 3.0]),
                 ("PEPTIDEK", 700.0, 2, [], [])])


def _c_nonfinite():
    aa, const = params_of()
    y1, y2 = fast_mass("K", "y", 1, aa, const), fast_mass("EK", "y", 1, aa, const)
    nan, inf = float("nan"), float("inf")
    s = "PEPTIDEK"
    return pack([(s, 700.0, 2, [y1, 300.0, 500.0], [1.0, nan, 2.0]),         # NaN inside the range: 0.0
                 (s, 700.0, 2, [50.0, y1, 300.0], [nan, 1.0, 3.0]),          # outside: no effect
                 (s, 700.0, 2, [y1, y1 * (1 + 5e-6), 300.0], [9.0, nan, 3.0]),  # NaN wins its window: still 0.0
                 (s, 700.0, 2, [y1, 300.0], [inf, 3.0]),                     # inf / inf
                 (s, 700.0, 2, [y1, 300.0], [3.0, inf]),                     # 3 / inf
                 (s, 700.0, 2, [y1, y2, 300.0], [inf, inf, 1.0]),
                 (s, 700.0, 2, [y1, nan, 300.0], [1.0, 1.0, 1.0]),           # non-finite m/z: unresolved
                 (s, 700.0, 2, [y1, 300.0, inf], [1.0, 1.0, 1.0]),
                 (s, 700.0, 2, [-inf, y1, 300.0], [1.0, 1.0, 1.0]),
                 (s, nan, 2, [y1, 300.0], [1.0, 1.0]),                       # non-finite precursor
                 (s, inf, 0, [y1, 300.0], [1.0, 1.0]),
                 (s, 700.0, 2, [y1, 300.0], [1.0, 3.0])])


def _c_bad_sequences():
    aa, const = params_of()
    y1 = fast_mass("K", "y", 1, aa, const)
    mz, inten = [y1, 300.0], [1.0, 3.0]
    seqs = ["PEPXIDEK", "peptidek", "_(ac)PEPTIDEK_", "PEPTIDEK2", "B", "J", "O", "U", "Z", "X", "PEPTIDE K", "@[",
            "PEPTIDEK"]
    out = [(s, 700.0, 2, mz, inten) for s in seqs]
    out.append(("PEPXIDEK", float("nan"), 2, [float("nan")], [1.0]))  # invalid wins over unresolved
    return pack(out)


def _c_limits():
    rng = np.random.default_rng(7)
    long = peptide(rng, 257)
    mz, inten = fragment_spectrum(rng, long[:256], 2)
    return pack([(long, 700.0, 2, mz, inten), (long[:256], 700.0, 2, mz, inten), (long[:256], 700.0, 65, mz, inten),
                 ("X" * 300, 700.0, 2, mz, inten), (long[:100], 700.0, 64, mz, inten)])


def _c_unsorted_long():
    rng = np.random.default_rng(303)
    seq = peptide(rng, 30)
    out = [(seq, precursor_of(seq, 3), 3, *fragment_spectrum(rng, seq, 3, sort=False)),
           (seq, precursor_of(seq, 3), 3, *fragment_spectrum(rng, seq, 3, n_true=35, total=65)),
           (seq, precursor_of(seq, 3), 3, *fragment_spectrum(rng, seq, 3, n_true=116, total=5000)),
           (seq, precursor_of(seq, 2), 2, *fragment_spectrum(rng, seq, 2, n_true=58, total=2700, sort=False))]
    # the unsorted ones also hold exact duplicates (equal m/z, equal intensity): the lower index counts once
    for k in (0, 3):
        s, p, z, mz, inten = out[k]
        dup = rng.choice(len(mz), size=len(mz) // 10, replace=False)
        out[k] = (s, p, z, np.concatenate([mz, mz[dup]]), np.concatenate([inten, inten[dup]]))
    assert [len(o[3]) for o in out] == [88, 65, 5000, 2970]  # 3,000 at most, a few thousand
    return pack(out)


def _c_seams():
    """Fragment counts around the lane seams.  A peptide of L residues at charge z has
    2 (L - 1) max(1, z - 1) fragments, an even number: 2, 62, 64, 66, 126, 128, 130 (and 1,
    63, 64, 65 cleavage sites), and 64 = 2 * 16 * 2 at charge 3."""
    rng = np.random.default_rng(404)
    out = []
    for n, z in ((2, 2), (32, 2), (33, 2), (34, 2), (64, 2), (65, 2), (66, 2), (17, 3), (2, 1)):
        seq = peptide(rng, n)
        out.append((seq, precursor_of(seq, z), z, *fragment_spectrum(rng, seq, z, n_true=130, n_noise=30)))
    return pack(out)  # nine segments: not a multiple of the kernel's four waves per workgroup


def _c_overlap():
    """Segments that overlap, repeat, are empty, reversed or outside the array, in any order."""
    rng = np.random.default_rng(505)
    seq = peptide(rng, 12)
    mz, inten = fragment_spectrum(rng, seq, 2, n_true=22, n_noise=128)
    n = len(mz)
    begin = np.array([0, 50, 0, 120, 10, -1, 0, 100, n, 0], np.int64)
    end = np.array([100, n, n, 120, 5, 5, n + 1, n, n, 100], np.int64)
    S = len(begin)
    return dict(mz=mz, inten=inten, seg_begin=begin, seg_end=end, prec_mz=np.full(S, precursor_of(seq, 2)),
                charge=np.full(S, 2, np.int32), peptides=[seq] * S, params={})


def _c_fuzz(seed):
    rng = np.random.default_rng(9000 + seed)
    out = []
    for _ in range(11):
        seq = peptide(rng, int(rng.integers(2, 41)))
        z = int(rng.integers(1, 6))
        prec = precursor_of(seq, z) * (1 + rng.normal(0, 5e-6))
        mz, inten = fragment_spectrum(rng, seq, z, n_true=int(rng.integers(0, 80)), n_noise=int(rng.integers(0, 300)),
                                      jitter_ppm=25.0, sort=bool(rng.integers(0, 4)))
        if len(mz) and rng.random() < 0.5:  # the precursor's own peaks, and a zero
            mz = np.concatenate([mz, [prec]])
            inten = np.concatenate([inten, [1e4]])
            order = np.argsort(mz, kind="stable")
            mz, inten = mz[order], inten[order]
            inten[int(rng.integers(0, len(inten)))] = 0.0
        out.append((seq, prec, z, mz, inten))
    return pack(out)


# changed parameters (a residue mass, 20 ppm, another range) over the fuzz spectra
PARAM_SETS = {"mass": {"K": 128.2}, "ppm20": {"tol_ppm": 20.0}, "range": {"min_mz": 200.0, "max_mz": 900.0},
              "proton": {"proton": 1.008, "precursor_proton": 1.007}}

CASES = {"lengths_charges": _c_lengths_charges, "window": _c_window, "shared_tied": _c_shared_tied,
         "tie_union": _c_tie_union, "precursor": _c_precursor, "range_ends": _c_range_ends,
         "empty_zero": _c_empty_zero, "nonfinite": _c_nonfinite, "bad_sequences": _c_bad_sequences,
         "limits": _c_limits, "unsorted_long": _c_unsorted_long, "seams": _c_seams, "overlap": _c_overlap}
CASES.update({f"fuzz{k}": functools.partial(_c_fuzz, k) for k in range(N_FUZZ)})
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("params_"):
        return dict(case("fuzz0"), params=PARAM_SETS[name[len("params_"):]])
    return CASES[name]()


def segments(c):
    """(index, peptide, prec_mz, charge, mz, inten) of the case's segments with a valid range."""
    n = len(c["mz"])
    for i, (b, e) in enumerate(zip(c["seg_begin"], c["seg_end"])):
        if 0 <= b <= e <= n:
            yield i, c["peptides"][i], float(c["prec_mz"][i]), int(c["charge"][i]), c["mz"][b:e], c["inten"][b:e]


@functools.lru_cache(maxsize=None)
def expect(name):
    """(fraction [S], status [S]) of a case by the restatement; computed once, never changed."""
    c = case(name)
    S = len(c["seg_begin"])
    fraction, status = np.full(S, np.nan), np.full(S, STATUS_UNRESOLVED, np.int32)
    for i, seq, prec, z, mz, inten in segments(c):
        fraction[i], status[i] = restate(seq, prec, z, mz, inten, c["params"])
    fraction.setflags(write=False)
    status.setflags(write=False)
    return fraction, status


# ------------------------------------------------------------------ best_by_explained
class Spectrum:
    def __init__(self, mz, intensity, precursor_mz, precursor_charge):
        self.mz, self.intensity = np.asarray(mz, np.float64), np.asarray(intensity, np.float64)
        self.precursor_mz, self.precursor_charge = precursor_mz, precursor_charge


@functools.lru_cache(maxsize=None)
def best_clusters():
    """(clusters of Spectrum, peptides): members with more or fewer of the peptide's fragments,
    an exact duplicate of the best one behind it, an empty cluster, a single member, and a
    cluster whose peptide is invalid (every fraction 0.0: the first member)."""
    rng = np.random.default_rng(606)
    clusters, peptides = [], []
    for n_members in (5, 1, 0, 9, 3, 4):
        seq = peptide(rng, int(rng.integers(7, 25)))
        z = int(rng.integers(2, 4))
        prec = precursor_of(seq, z)
        members = [Spectrum(*fragment_spectrum(rng, seq, z, n_true=int(rng.integers(3, 40)), n_noise=60), prec, z)
                   for _ in range(n_members)]
        clusters.append(members)
        peptides.append(seq)
    fr = [restate(peptides[3], s.precursor_mz, s.precursor_charge, s.mz, s.intensity)[0] for s in clusters[3]]
    top = clusters[3][int(np.argmax(fr))]
    clusters[3].append(Spectrum(top.mz.copy(), top.intensity.copy(), top.precursor_mz, top.precursor_charge))
    peptides[5] = "PEPTIDEX"
    return clusters, peptides


@functools.lru_cache(maxsize=None)
def best_expect():
    """(indices, fractions per cluster) by the restatement: np.argmax = first among equals."""
    clusters, peptides = best_clusters()
    fractions = [np.array([restate(p, s.precursor_mz, s.precursor_charge, s.mz, s.intensity)[0] for s in cl])
                 for cl, p in zip(clusters, peptides)]
    return [int(np.argmax(f)) if len(f) else -1 for f in fractions], fractions
