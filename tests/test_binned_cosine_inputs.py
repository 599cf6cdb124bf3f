"""CPU checks of the binned-cosine edge cases (tests/binned_cosine_cases.py): the numpy
oracle equals the reference's own cos_dist / average_cos_dist on every case
(tests/golden/binned_cosine_edges.npz), every named case has the property it is named
for, and the cases whose point is one clause of the kernel are sensitive to it: a
model of the pair with that clause wrong differs from the oracle far beyond the
tolerance tests/test_gpu_cosine.py compares with."""
import os

import numpy as np
import pytest

import binned_cosine_cases as cases
from conftest import GOLDEN

SENSITIVE = 1e-6  # relative; the GPU tests compare at cases.RTOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "binned_cosine_edges.npz"))


# ------------------------------------------------------------ a model of one pair
def pair_bins(mz, max_mz, s, on_edge=True):
    """Per peak of one spectrum under the pair's cut: (bin or -1, raw bin, on-edge?, kc).
    Bins by np.digitize on the pair's own edges, as scipy's binned_statistic."""
    mz = np.asarray(mz, np.float64)
    edges = np.arange(-s / 2., max_mz, s)
    kc = len(edges) - 2
    dec = int(-np.log10(np.diff(edges).min())) + 6
    raw = np.digitize(mz, edges) - 1
    on = (mz >= edges[-1]) & (np.around(mz, dec) == np.around(edges[-1], dec))
    b = np.where((raw >= 0) & (raw <= kc), raw, -1)
    if on_edge:
        b[on] = kc
    return b, raw, on, kc


def _stretches(b):
    """Maximal stretches [i, j) of peaks of one valid bin with no other valid bin between
    (invalid peaks inside do not end a stretch: np.bincount sums them as one bin)."""
    out, i = [], 0
    valid = [q for q in range(len(b)) if b[q] >= 0]
    while i < len(valid):
        j = i
        while j + 1 < len(valid) and b[valid[j + 1]] == b[valid[i]]:
            j += 1
        out.append(valid[i:j + 1])
        i = j + 1
    return out


def model_cos(rep, mem, s, on_edge=True, runs="exact"):
    """cos_dist of one pair from sparse sums.  ``runs`` is how B.B is formed: "exact"
    (one sum per bin), "split" (an invalid peak between two peaks of a bin ends the run),
    "drop_carry" (a run that reaches the last peak of a 64-peak chunk with more peaks to
    come loses what it has summed so far).  ``on_edge=False`` drops the shift of
    rightmost-edge peaks into the last bin."""
    max_mz = max(rep[0][-1], mem[0][-1])
    rbins = pair_bins(rep[0], max_mz, s, on_edge)[0]
    mbins = pair_bins(mem[0], max_mz, s, on_edge)[0]
    A = {}
    for b, I in zip(rbins, rep[1]):
        if b >= 0:
            A[b] = A.get(b, 0.0) + I
    aa = sum(v * v for _, v in sorted(A.items()))
    ab = sum(I * A.get(b, 0.0) for b, I in zip(mbins, mem[1]) if b >= 0)
    if runs == "exact":
        B = {}
        for b, I in zip(mbins, mem[1]):
            if b >= 0:
                B[b] = B.get(b, 0.0) + I
        bb = sum(v * v for v in B.values())
    else:
        bb, m = 0.0, len(mbins)
        for st in _stretches(mbins):
            pieces = [[st[0]]]
            for q in st[1:]:
                gap = q != pieces[-1][-1] + 1
                if runs == "split" and gap:
                    pieces.append([q])
                else:
                    pieces[-1].append(q)
            if runs == "split":
                bb += sum(sum(mem[1][q] for q in p) ** 2 for p in pieces)
            else:
                acc = 0.0
                for q in st:
                    acc += mem[1][q]
                    if q % cases.WAVE == cases.WAVE - 1 and q + 1 < m:
                        acc = 0.0  # the carry dropped
                bb += acc * acc
    if aa == 0.0 or bb == 0.0:
        return 0.0
    return ab / np.sqrt(aa * bb)


def _pairs(name):
    cos = cases.expect(name)[0]
    k = 0
    for c, (members, rep) in enumerate(cases.clusters_of(name)):
        for j, mem in enumerate(members):
            yield c, j, rep, mem, cos[k]
            k += 1


def _rel(a, b):
    return abs(a - b) / abs(b)


# ------------------------------------------------- the oracle equals the reference
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_oracle_matches_reference_golden(golden, name):
    csr, rep_off, rep_mz, rep_int, s, want = cases.golden_case(golden, name)
    mine = cases.to_csr(name)
    assert s == cases.mz_space_of(name)
    for a, b in zip((csr.cluster_off, csr.spec_off, csr.mz, csr.inten, rep_off, rep_mz, rep_int),
                    (mine[0].cluster_off, mine[0].spec_off, mine[0].mz, mine[0].inten) + mine[1:]):
        np.testing.assert_array_equal(a, b)  # the committed inputs are the generator's (NaN == NaN here)
    cos, avg, status = cases.expect(name)
    np.testing.assert_array_equal(status, want[2])
    np.testing.assert_allclose(cos, want[0], rtol=cases.RTOL, atol=0, equal_nan=True)
    np.testing.assert_allclose(avg, want[1], rtol=cases.RTOL, atol=0, equal_nan=True)


def test_golden_holds_every_case_once(golden):
    assert sorted(golden["case_names"]) == sorted(cases.CASES)
    assert golden["case_off"][-1] == len(golden["cluster_off"]) - 1


@pytest.mark.parametrize("name", ["rep_on_edge", "high_mz", "chunk_runs", "sandwiched", "mz_space_0.02", "mz_space_1.0005"])
def test_model_equals_oracle(name):
    """The model the property and sensitivity checks below rest on is the oracle's
    computation (finite cases)."""
    for c, j, rep, mem, want in _pairs(name):
        assert model_cos(rep, mem, cases.mz_space_of(name)) == pytest.approx(want, rel=1e-12), (c, j)


# ------------------------------------------------------------------ rep_on_edge
def _roe(variant):
    members, rep = cases.clusters_of("rep_on_edge")[cases.ROE_VARIANTS.index(variant)]
    return members, rep


def _rep_view(rep, mem, s=cases.MZ_SPACE):
    return pair_bins(rep[0], max(rep[0][-1], mem[0][-1]), s)


@pytest.mark.parametrize("variant", cases.ROE_VARIANTS)
def test_rep_on_edge_properties(variant):
    members, rep = _roe(variant)
    mem = members[0]
    assert mem[0][-1] > rep[0].max()  # the member supplies the pair's maximum
    b, raw, on, kc = _rep_view(rep, mem)
    # two peaks past the last edge that round onto it, one that does not
    assert (raw == kc + 1).sum() == 3 and (on & (raw == kc + 1)).sum() == 2 and (b == -1).sum() == 1
    has_kc = bool(np.any(raw == kc))
    assert has_kc == (variant in ("a", "c", "d", "e", "f_a"))
    mb = pair_bins(mem[0], mem[0][-1], cases.MZ_SPACE)[0]
    assert bool(np.any(mb == kc)) == (variant in ("e", "d", "f_e"))
    assert (kc >= cases.TABLE_BINS) == variant.startswith("f")
    if variant == "c":  # unsorted: an on-edge peak, the bin-kc peak, the other on-edge peak, in input order
        assert np.any(np.diff(rep[0]) < 0)
        pos_on, pos_kc = np.flatnonzero(on), np.flatnonzero(raw == kc)
        assert pos_on[0] < pos_kc[0] < pos_on[1]
        assert np.any(pair_bins(members[1][0], members[1][0][-1], cases.MZ_SPACE)[0] == kc)
    if variant == "d":  # the second member ends higher: the same peaks are ordinary bins there
        b2, raw2, on2, kc2 = _rep_view(rep, members[1])
        assert kc2 > kc + 1 and not on2.any() and np.all(b2 >= 0) and (b2 == kc + 1).sum() == 3
        assert np.any(pair_bins(members[1][0], members[1][0][-1], cases.MZ_SPACE)[0] == kc + 1)


def test_rep_on_edge_is_sensitive_to_the_shift():
    worst = {}
    for c, j, rep, mem, want in _pairs("rep_on_edge"):
        worst[(c, j)] = _rel(model_cos(rep, mem, cases.MZ_SPACE, on_edge=False), want)
    d = cases.ROE_VARIANTS.index("d")
    assert all(v > SENSITIVE for k, v in worst.items() if k != (d, 1)), worst
    assert worst[(d, 1)] == 0.0  # no on-edge peak in that pair


# ---------------------------------------------------------------------- high_mz
def test_high_mz_properties():
    cl = cases.clusters_of("high_mz")
    lens = [len(rep[0]) for _, rep in cl]
    assert lens[0] <= cases.RCAP and lens[1] <= cases.RCAP < lens[2]
    assert [bool(np.any(np.diff(rep[0]) < 0)) for _, rep in cl] == [False, True, False]
    assert cl[1][1][0][-1] < cl[1][1][0].max()
    seam = set(cases.HIGH_SEAM)
    assert min(seam) < cases.TABLE_BINS <= max(seam)
    only_rep = only_mem = 0
    for c, j, rep, mem, want in _pairs("high_mz"):
        assert len(mem[0]) <= 70 and 0.0 < want < 1.0
        max_mz = max(rep[0][-1], mem[0][-1])
        rb, _, _, kc = pair_bins(rep[0], max_mz, cases.MZ_SPACE)
        mb = pair_bins(mem[0], max_mz, cases.MZ_SPACE)[0]
        assert kc >= cases.TABLE_BINS
        for mz, b in ((rep[0], rb), (mem[0], mb)):  # mid-bin: no peak near an edge
            fr = (mz - np.array([cases.edge(int(k)) for k in np.digitize(mz, np.arange(-cases.MZ_SPACE / 2., mz.max() + 1, cases.MZ_SPACE)) - 1])) / cases.MZ_SPACE
            assert np.all((fr > 0.4) & (fr < 0.8))
        shared = set(rb[rb >= 0]) & set(mb[mb >= 0])
        assert any(b < cases.TABLE_BINS for b in shared) and any(b >= cases.TABLE_BINS for b in shared)
        assert sum(3000.0 < cases.edge(int(b)) < 4500.0 for b in shared) >= 3
        assert shared & seam
        only_rep += bool((set(rb[rb >= 0]) - set(mb[mb >= 0])) & seam)
        only_mem += bool((set(mb[mb >= 0]) - set(rb[rb >= 0])) & seam)
    assert only_rep >= 2 and only_mem >= 2  # a seam bin on one side only, both ways


# ------------------------------------------------------------------- chunk_runs
def test_chunk_runs_properties():
    (members, rep), = cases.clusters_of("chunk_runs")
    assert [(len(m[0]), r0, rl) for m, (_, r0, rl) in zip(members, cases.CHUNK_RUNS)] == list(cases.CHUNK_RUNS)
    want = {0: (10, 139), 1: (60, 63), 2: (120, 127), 3: (64, 127), 4: (60, 63), 5: (120, 127), 6: (60, 64)}
    rbins = set(pair_bins(rep[0], rep[0][-1], cases.MZ_SPACE)[0])
    for k, mem in enumerate(members):
        assert rep[0][-1] > mem[0].max()
        b = pair_bins(mem[0], rep[0][-1], cases.MZ_SPACE)[0]
        assert np.all(b >= 0) and np.all(np.diff(b) >= 0) and np.all(np.diff(mem[0]) > 0)
        long = [st for st in _stretches(b) if len(st) > 1]
        assert len(long) == 1 and (long[0][0], long[0][-1]) == want[k]
        assert b[long[0][0]] in rbins                       # A.B sees the run
        assert len(set(mem[1])) == len(mem[1])              # distinct intensities
    assert [len(m[0]) for m in members][4:] == [64, 128, 65]
    assert want[4][1] == 63 and want[5][1] == 127 and want[6][1] == 64   # each ends in its run
    assert want[0][1] - want[0][0] + 1 == 130 and want[1][1] % 64 == 63 and want[3] == (64, 127)


def test_chunk_runs_are_sensitive_to_the_carry():
    diff = [_rel(model_cos(rep, mem, cases.MZ_SPACE, runs="drop_carry"), want) for _, _, rep, mem, want in _pairs("chunk_runs")]
    # the 64-peak member has one chunk and carries nothing (the 128-peak one carries the
    # one-peak run at position 63)
    assert [d > SENSITIVE for d in diff] == [True, True, True, True, False, True, True], diff


# ------------------------------------------------------------------- sandwiched
def test_sandwiched_properties():
    (members, rep), = cases.clusters_of("sandwiched")
    assert rep[0][-1] == cases.SANDWICH_REP_LAST
    assert [p for p, _ in cases.SANDWICHED] == [1, 1, 11, 11, 64, 64, 63, 63, 1]
    np.testing.assert_array_equal(members[0][0], [500.0, 1999.0, 500.001, 1000.0])
    for mem, (pos, kind) in zip(members, cases.SANDWICHED):
        max_mz = max(rep[0][-1], mem[0][-1])
        b = pair_bins(mem[0], max_mz, cases.MZ_SPACE)[0]
        assert b[pos] == -1 and b[pos - 1] == b[pos + 1] >= 0 and (b == -1).sum() == 1
        valid = b[b >= 0]
        assert np.all(np.diff(valid) >= 0)  # nothing else sends the member to the unsorted pass
        assert b[pos - 1] in set(pair_bins(rep[0], max_mz, cases.MZ_SPACE)[0])
        x = mem[0][pos]
        if kind == "above":  # above the cut: larger than both last m/z, so the member is unsorted in m/z
            assert x > max_mz and np.any(np.diff(mem[0]) < 0)
        elif kind == "below":
            assert x == -1.0 < -cases.MZ_SPACE / 2.
        else:
            assert np.isnan(x)


def test_sandwiched_is_sensitive_to_split_runs():
    diff = [_rel(model_cos(rep, mem, cases.MZ_SPACE, runs="split"), want) for _, _, rep, mem, want in _pairs("sandwiched")]
    assert all(d > SENSITIVE for d in diff), diff


# ---------------------------------------------------------------- many_deferred
def test_many_deferred_properties():
    cl = cases.clusters_of("many_deferred")
    assert len(cl) == cases.N_DEFERRED_CLUSTERS == 72
    R = np.array([len(rep[0]) for _, rep in cl])
    assert R.max() == 640 and R.min() == cases.RCAP + 1 and np.all(np.diff(R) < 0)
    status = cases.expect("many_deferred")[2]
    n_members = np.array([len(m) for m, _ in cl])
    empty_member = np.array([any(len(x[0]) == 0 for x in m) for m, _ in cl])
    # deferred: scored from the global scratch (no members / an empty member never get there)
    deferred = (R > cases.RCAP) & (n_members > 0) & ~empty_member
    assert deferred.sum() == 70 > cases.FALLBACK_BLOCKS
    assert (n_members == 0).sum() == 1 and empty_member.sum() == 1
    np.testing.assert_array_equal(status, np.where(empty_member, cases.STATUS_EMPTY, cases.STATUS_OK))
    unsorted = [bool(np.any(np.diff(rep[0]) < 0)) for _, rep in cl]
    assert unsorted == [c % 10 == 5 for c in range(72)]
    for members, rep in cl:
        assert rep[0].min() >= 100.0 and rep[0].max() <= 300.0
        assert all(len(m[0]) in (0, 20) and (len(m[0]) == 0 or (m[0].min() > 99.0 and m[0].max() < 301.0)) for m in members)
    cos = cases.expect("many_deferred")[0]
    assert np.nanmin(cos) > 0.0 and np.isnan(cos).sum() == 2


def test_rcap_boundary_properties():
    cl = cases.clusters_of("rcap_boundary")
    assert [len(rep[0]) for _, rep in cl] == [cases.RCAP - 1, cases.RCAP, cases.RCAP + 1] == list(cases.RCAP_LENGTHS)
    for (members, rep), (m2, rep2) in zip(cl[:-1], cl[1:]):
        np.testing.assert_array_equal(rep[0], rep2[0][:-1])
        np.testing.assert_array_equal(rep[1], rep2[1][:-1])
        for a, b in zip(members, m2):
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
    assert all(m[0][-1] > cl[-1][1][0].max() for m in cl[0][0])  # the members set the cut
    cos = cases.expect("rcap_boundary")[0].reshape(3, -1)
    assert np.all(cos > 0.0) and not np.array_equal(cos[0], cos[2])  # the extra peaks count


def test_unresolved_case_properties():
    cl = cases.clusters_of("unresolved")
    R = [len(rep[0]) for _, rep in cl]
    assert R == list(cases.UNRESOLVED_LENGTHS) and sum(r > cases.UNRESOLVED_MAX_REP for r in R) == 1
    assert cases.RCAP + 1 in R and min(R) < cases.RCAP < cases.UNRESOLVED_MAX_REP
    assert np.all(cases.expect("unresolved")[2] == cases.STATUS_OK)


# --------------------------------------------------------------------- mz_space
@pytest.mark.parametrize("s", cases.SPACINGS)
def test_mz_space_properties(s):
    name = f"mz_space_{s}"
    assert cases.mz_space_of(name) == s
    cl = cases.clusters_of(name)
    (mem,), rep = cl[1]  # an on-edge member: the representative supplies the maximum
    assert rep[0][-1] > mem[0][-1]
    b, raw, on, kc = pair_bins(mem[0], rep[0][-1], s)
    assert list(on) == [False, False, True, True, False] and list(raw[2:]) == [kc + 1] * 3 and b[4] == -1
    assert np.any(pair_bins(rep[0], rep[0][-1], s)[0] == kc)
    (mem,), rep = cl[2]  # an on-edge representative
    b, raw, on, kc = _rep_view(rep, mem, s)
    assert (on & (raw == kc + 1)).sum() == 2 and (b == -1).sum() == 1 and np.any(raw == kc)
    for c, j, rep, mem, want in _pairs(name):
        if c > 0:
            assert _rel(model_cos(rep, mem, s, on_edge=False), want) > SENSITIVE
    # the decimals of the on-edge rounding differ between the spacings
    dec = {x: int(-np.log10(np.diff(np.arange(-x / 2., 900.0, x)).min())) + 6 for x in cases.SPACINGS}
    assert dec == {0.005: 8, 0.02: 7, 0.1: 7, 1.0005: 6}
    assert cases.decimals(s) == dec[s]


# -------------------------------------------------------------------- nonfinite
def test_nonfinite_expectations():
    """What the reference gives (the golden test above pins these to it): an infinite
    bin inside the cut against a non-zero partner is NaN; past the cut it is dropped;
    against an all-zero partner the result is 0.0; a square that overflows is 0.0."""
    cl = cases.clusters_of("nonfinite")
    cos, avg, status = cases.expect("nonfinite")
    assert np.all(status == cases.STATUS_OK)
    off = np.concatenate([[0], np.cumsum([len(m) for m, _ in cl])])
    got = [list(cos[off[c]:off[c + 1]]) for c in range(len(cl))]
    n = np.isnan
    assert n(got[0]).all() and n(got[1]).all()
    assert got[2] == [0.5] and got[3] == [pytest.approx(0.5 ** 0.5)]
    assert n(got[4]).all() and len(got[4]) == 3
    assert n(got[5]).all() and n(got[6][0]) and got[6][1] == pytest.approx(0.5 ** 0.5)
    assert n(got[7]).all() and n(got[8]).all()
    assert got[9][0] == 0.0 and n(got[9][1]) and got[10] == [0.0]
    assert got[11] == [0.0] and got[12] == [0.0] and got[13] == [0.5]
    assert n(got[14]).all() and n(got[15]).all() and n(got[16]).all()
    assert n(got[17][0]) and n(got[17][2]) and got[17][1] == pytest.approx(got[17][3], rel=1e-14) and got[17][1] > 0.1
    assert n(got[18]).all() and not n(got[19]).any() and min(got[19]) > 0.0
    # where the infinities sit
    assert not np.isfinite(cl[2][1][1][-1]) and cl[2][1][0][-1] == cl[2][1][0].max()
    assert cl[3][1][0][-1] < cl[3][1][0].max()
    for c in (11, 12, 13, 14, 15):  # finite inputs only
        assert all(np.all(np.isfinite(i)) for _, i in cl[c][0]) and np.all(np.isfinite(cl[c][1][1]))
    b, raw, on, kc = _rep_view(cl[16][1], cl[16][0][0])
    assert np.isinf(cl[16][1][1][on]).sum() == 1 and np.all(np.isfinite(cl[16][1][1][raw == kc]))
    m17 = cl[17][0]
    assert len(m17[0][0]) > cases.WAVE and np.isinf(m17[0][1][62]) and np.all(np.diff(m17[0][0]) > 0)
    assert np.any(np.diff(m17[2][0]) < 0) and np.isinf(m17[2][1]).sum() == 1
    assert len(cl[18][1][0]) > cases.RCAP and len(cl[19][1][0]) > cases.RCAP
    assert np.isinf(cl[19][1][1][-1]) and np.isinf(cl[18][1][1]).sum() == 1
