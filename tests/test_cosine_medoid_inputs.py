"""CPU checks of the cosine medoid's oracle and inputs (tests/cosine_medoid_cases.py):
the composition over oracle/np_oracle.py equals the reference's own
average_cos_dist (tests/golden/cosine_medoid.npz), every named case has the property
it is named for, and no committed cluster's best and runner-up scores fall between
"bitwise equal" and "1e-9 apart", so tests/test_gpu_cosine_medoid.py can demand exact
indices everywhere.  Also: the new entry points are declared and exported."""
import ctypes
import getopt

import numpy as np
import pytest

import cosine_medoid_cases as cases
from conftest import load_golden
from oracle import np_oracle
from specpride_amd import _lib, engine
from specpride_amd import most_similar_representative as msr


def test_composition_matches_reference_golden():
    z, csr = load_golden("cosine_medoid.npz")
    clusters = cases.from_csr(csr)
    want = cases.golden_clusters()
    assert len(clusters) == len(want) == 12
    for a, b in zip(clusters, want):  # the committed inputs are the generator's
        assert len(a) == len(b)
        for (m1, i1), (m2, i2) in zip(a, b):
            np.testing.assert_array_equal(m1, m2)
            np.testing.assert_array_equal(i1, i2)
    assert sorted(len(c) for c in clusters)[:9] == [1, 2, 3, 3, 4, 5, 5, 6, 7]
    assert all(5 <= len(m) <= 40 for c in clusters for m, _ in c)
    assert float(z["mz_space"]) == cases.MZ_SPACE
    rep, score, status = cases.oracle(clusters, float(z["mz_space"]))
    np.testing.assert_array_equal(rep, z["rep"])
    np.testing.assert_allclose(score, z["score"], rtol=cases.RTOL, atol=0)
    assert np.all(status == cases.STATUS_OK)
    # ... and equals the helper's cached result for the named case
    np.testing.assert_array_equal(cases.expect("golden")[0], z["rep"])


def test_cos_dist_is_symmetric_bit_for_bit():
    """What lets the helper (and the kernel) evaluate each unordered pair once."""
    for members in cases.golden_clusters()[:6]:
        for i in range(len(members)):
            for j in range(i + 1, len(members)):
                a, b = members[i], members[j]
                assert np_oracle.cos_dist(a[0], a[1], b[0], b[1]) == np_oracle.cos_dist(b[0], b[1], a[0], a[1])


def _scores(name, c):
    cl = cases.clusters_of(name)
    rep, score, status = cases.expect(name)
    first = sum(len(x) for x in cl[:c])
    return rep[c] - first if rep[c] >= 0 else -1, score[first:first + len(cl[c])], status[c]


def test_small_and_zero_clusters():
    cl = cases.clusters_of("small")
    assert [len(c) for c in cl] == [1, 2, 3, 2, 3]
    assert _scores("small", 0)[0] == 0
    r, s, _ = _scores("small", 1)  # n = 2 with non-zero norms: an exact tie, the first wins
    assert r == 0 and s[0] == s[1] and s[0] > 0.5
    r, s, _ = _scores("small", 3)  # member 0 all zero: every cosine with it is 0.0
    assert r == 1 and s[0] == 0.0 and s[1] == 0.5
    r, s, _ = _scores("small", 4)
    assert r == 0 and np.all(s == 0.0)


def test_duplicates_tie_exactly_and_the_first_wins():
    r, s, _ = _scores("duplicates", 0)  # [a, b, c, a, d, a]
    assert r == 0 and s[0] == s[3] == s[5] and s[0] > max(s[1], s[2], s[4])
    r, s, _ = _scores("duplicates", 1)  # [b, a, c, d, a]
    assert r == 1 and s[1] == s[4] and s[1] > max(s[0], s[2], s[3])


def test_per_pair_cut_cases():
    cl = cases.clusters_of("cut")
    lasts = [m[-1] for m, _ in cl[0]]
    assert 499 < min(lasts) < 502 and 1499 < max(lasts) < 1502
    # a one-peak spectrum: its only peak lies past the last edge of its own cut
    assert np_oracle.cos_dist(*cl[2][0], *cl[2][0]) == 0.0
    assert np.all(_scores("cut", 1)[1] == 0.0) and _scores("cut", 2)[0] == 0
    # one ulp above an edge: the on-edge rule moves the top peak into the last bin
    x = cl[3][0][0][-1]
    edges = np.arange(-cases.MZ_SPACE / 2., x, cases.MZ_SPACE)
    assert x > edges[-1] and x == np.nextafter(edges[-1], np.inf)
    kept = np_oracle.bin_proc(*cl[3][0], cases.MZ_SPACE, x)
    assert kept[-1] == 3.0 and _scores("cut", 3)[1][0] == 1.0
    assert cl[4][0][0][-1] == cl[4][1][0][-1] == x and _scores("cut", 4)[2] == cases.STATUS_OK


def test_order_and_validity_cases():
    cl = cases.clusters_of("order")
    mz = cl[0][1][0]
    assert mz[-1] != mz.max() and np.any(np.diff(mz) < 0)
    dense = cl[1][0][0]
    bins = np.floor((dense + cases.MZ_SPACE / 2.) / cases.MZ_SPACE)
    assert len(np.unique(bins)) < len(bins) / 2
    assert any(np.isnan(m).any() for m, _ in cl[2]) and any((m < 0).any() for m, _ in cl[2])
    assert all(np.isfinite(m[-1]) for m, _ in cl[2])
    assert np.all(cases.expect("order")[2] == cases.STATUS_OK)


def test_empty_cases():
    rep, score, status = cases.expect("empty")
    assert list(status) == [3, 0, 3, 0, 3, 0, 3]
    assert list(rep >= 0) == [False, True, False, False, False, True, False]
    assert np.isnan(score[:3]).all() and not np.isnan(score[3:5]).any()


def test_seam_cases_sit_on_the_published_caps():
    assert (cases.LDS_MEMBERS, cases.LDS_RUNS) == (engine.COSINE_MEDOID_LDS_MEMBERS, engine.COSINE_MEDOID_LDS_RUNS)
    assert [len(c) for c in cases.clusters_of("member_seams")] == [64, 65, 130]
    for cl, k in zip(cases.clusters_of("run_seams"), (63, 64, 65)):
        for m, _ in cl:  # every peak in a bin of its own
            assert len(np.unique(np.floor((m + cases.MZ_SPACE / 2.) / cases.MZ_SPACE))) == len(m) == k
    at, past = cases.clusters_of("lds_runs")
    assert sum(len(m) for m, _ in at) == cases.LDS_RUNS and sum(len(m) for m, _ in past) == cases.LDS_RUNS + 1
    big = cases.clusters_of("long_spectrum")[0]
    assert [len(m) for m, _ in big] == [50, 5000, 50] and np.all(np.diff(big[1][0]) >= 0)
    assert max(len(c) for k in range(cases.N_FUZZ) for c in cases.clusters_of(f"fuzz{k}")) <= 40
    assert max(len(m) for k in range(cases.N_FUZZ) for c in cases.clusters_of(f"fuzz{k}") for m, _ in c) <= 120


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_tie_condition(name):
    """Best and runner-up are bitwise equal for a structural reason (n = 2, a duplicated
    member, or no non-zero cosine at all) or more than 1e-9 relative apart."""
    cl = cases.clusters_of(name)
    rep, score, status = cases.expect(name)
    first = 0
    for c, members in enumerate(cl):
        n = len(members)
        if status[c] == cases.STATUS_OK and n >= 2:
            s = np.sort(score[first:first + n])[::-1]
            if s[0] == s[1]:
                best = [i for i in range(n) if score[first + i] == s[0]]
                a, b = members[best[0]], members[best[1]]
                dup = np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                assert n == 2 or dup or s[0] == 0.0, (name, c)
            else:
                assert (s[0] - s[1]) > cases.TIE_GAP * abs(s[0]), (name, c, s[0], s[1])
        first += n


def test_entry_points_declared_and_exported():
    assert {"spx_cosine_medoid", "spx_cosine_medoid_workspace_size"} <= set(_lib.EXPORTED)
    L = ctypes.CDLL(_lib.build())  # cross-compiles for gfx950 when stale; no GPU needed
    assert hasattr(L, "spx_cosine_medoid") and hasattr(L, "spx_cosine_medoid_workspace_size")
    L.spx_cosine_medoid_workspace_size.restype = ctypes.c_size_t
    L.spx_cosine_medoid_workspace_size.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    csr = _lib.SpxCsr(3, 10, 1000, None, None, None, None, None, None, None)
    info = _lib.SpxBatchInfo(500, 4, 0.0)
    small = L.spx_cosine_medoid_workspace_size(ctypes.byref(csr), ctypes.byref(info))
    csr.n_peaks = 2000
    # 28 B a peak (three f64 arrays and one i32, each 256-aligned)
    assert L.spx_cosine_medoid_workspace_size(ctypes.byref(csr), ctypes.byref(info)) - small >= 28 * 1000 - 4 * 256
    assert L.spx_cosine_medoid_workspace_size(None, ctypes.byref(info)) == 0


def test_cli_method_option(capsys):
    """-m takes xcorr or cosine; anything else prints the usage line and exits 2 before
    any file is touched."""
    for argv in (["-i", "x.mgf", "-o", "y.mgf", "-m", "bogus"], ["-m"]):
        with pytest.raises(SystemExit) as e:
            msr.main(argv)
        assert e.value.code == 2
        assert capsys.readouterr().out == "most_similar_representative.py -i <inputfile> -o <outputfile>\n"
    assert msr.METHODS == ("xcorr", "cosine")
    assert getopt.getopt(["-m", "cosine"], "hi:o:m:")[0] == [("-m", "cosine")]
