"""GPU parity of the binned-cosine evaluation (spx_binned_cosine) against the
reference's own benchmark.cos_dist / average_cos_dist outputs (golden) and the
numpy restatement (oracle/np_oracle.py).  Bar: statuses exact, cosines and
averages within 1e-12 relative (the reference sums its dot products in BLAS
order; the north star allows 1e-5)."""
from types import SimpleNamespace

import numpy as np
import pytest

import binned_cosine_cases as cases
from conftest import load_golden
from oracle import np_oracle
from specpride_amd import benchmark, engine
from specpride_amd.csr import SpectraCSR
from specpride_amd.synthetic import make_clusters_np

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _run(csr, rep_off, rep_mz, rep_int, mz_space=np_oracle.MZ_SPACE):
    b = engine.DeviceBatch.from_host(csr)
    return engine.binned_cosine(b, _dev(rep_off), _dev(rep_mz if len(rep_mz) else np.zeros(1)),
                                _dev(rep_int if len(rep_int) else np.zeros(1)), mz_space=mz_space).to_host()


def _check(got, want, n_clusters, n_spectra):
    cos, avg, st = got
    wcos, wavg, wst = want
    np.testing.assert_array_equal(st[:n_clusters], wst)
    np.testing.assert_allclose(cos[:n_spectra], wcos, rtol=RTOL, atol=0, equal_nan=True)
    np.testing.assert_allclose(avg[:n_clusters], wavg, rtol=RTOL, atol=0, equal_nan=True)


def test_binned_cosine_matches_reference_golden(gpu):
    z, csr = load_golden("binned_cosine.npz")
    got = _run(csr, z["rep_off"], z["rep_mz"], z["rep_int"], float(z["mz_space"]))
    _check(got, (z["cos"], z["avg"], z["status"]), csr.n_clusters, csr.n_spectra)


def _shuffled_members(csr, seed=5):
    rng = np.random.default_rng(seed)
    mz, it = csr.mz.copy(), csr.inten.copy()
    for s in range(0, csr.n_spectra, 5):
        a, b = csr.spec_off[s], csr.spec_off[s + 1]
        p = rng.permutation(b - a)
        mz[a:b], it[a:b] = mz[a:b][p], it[a:b][p]
    return SpectraCSR(csr.cluster_off, csr.spec_off, mz, it, csr.prec_mz, csr.charge, csr.rt)


@pytest.mark.parametrize("rep_kind", ["bin_mean", "medoid"])
def test_binned_cosine_synthetic_vs_oracle(gpu, rep_kind):
    """Representatives as the pipeline makes them: the bin-mean consensus
    (compacted engine output) or the medoid spectrum; every fifth member
    unsorted (the O(m^2) B.B path)."""
    csr = make_clusters_np(50, seed=77)
    b = engine.DeviceBatch.from_host(csr)
    if rep_kind == "bin_mean":
        r = engine.bin_mean(b).to_host()
        rep_off, rep_mz, rep_int = r["out_off"], r["out_mz"], r["out_int"]
    else:
        rep, _ = engine.medoid(b).to_host()
        lens = csr.spec_off[rep + 1] - csr.spec_off[rep]
        rep_off = np.concatenate([[0], np.cumsum(lens)])
        rep_mz = np.concatenate([csr.mz[csr.spec_off[s]:csr.spec_off[s + 1]] for s in rep])
        rep_int = np.concatenate([csr.inten[csr.spec_off[s]:csr.spec_off[s + 1]] for s in rep])
    mem = _shuffled_members(csr)
    got = _run(mem, rep_off, rep_mz, rep_int)
    want = np_oracle.binned_cosine(mem, rep_off, rep_mz, rep_int)
    _check(got, want, csr.n_clusters, csr.n_spectra)
    assert np.all(got[2][:csr.n_clusters] == 0) and np.all(got[1][:csr.n_clusters] > 0.0)


def test_binned_cosine_long_members_and_runs(gpu):
    """Members longer than a wave (runs carried across 64-peak chunks), many
    peaks per bin, a representative longer than the members."""
    rng = np.random.default_rng(3)
    clusters, reps = [], []
    for k in range(6):
        base = np.sort(rng.uniform(100, 1900, 40))
        members = []
        for _ in range(5 + k):
            mz = np.sort(np.concatenate([base + rng.normal(0, 0.0008, 40) for _ in range(5)]))  # 200 peaks, dense bins
            members.append({"m/z array": np.round(mz, 5), "intensity array": rng.lognormal(5, 1, len(mz))})
        clusters.append(members)
        rm = np.sort(np.concatenate([base, rng.uniform(100, 1990, 300)]))
        reps.append((rm, rng.lognormal(4, 1, len(rm))))
    csr = SpectraCSR.from_clusters(clusters)
    rep_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in reps])])
    rep_mz, rep_int = np.concatenate([r[0] for r in reps]), np.concatenate([r[1] for r in reps])
    _check(_run(csr, rep_off, rep_mz, rep_int), np_oracle.binned_cosine(csr, rep_off, rep_mz, rep_int),
           csr.n_clusters, csr.n_spectra)


def test_benchmark_shim_names(gpu):
    """specpride_amd.benchmark keeps the reference's function names (benchmark.py:19-38)."""
    a = SimpleNamespace(mz=np.array([200.0, 250.0, 900.0]), intensity=np.array([3.0, 4.0, 5.0]))
    b = SimpleNamespace(mz=np.array([200.001, 500.0]), intensity=np.array([1.0, 2.0]))
    assert benchmark.cos_dist(a, a) == pytest.approx(1.0, rel=1e-15)
    want = np_oracle.cos_dist(a.mz, a.intensity, b.mz, b.intensity)
    assert benchmark.cos_dist(a, b) == pytest.approx(want, rel=RTOL)
    assert benchmark.average_cos_dist(a, []) == 0.0
    assert benchmark.average_cos_dist(a, [a, b]) == pytest.approx((1.0 + want) / 2, rel=RTOL)
    with pytest.raises(IndexError):
        benchmark.cos_dist(a, SimpleNamespace(mz=np.zeros(0), intensity=np.zeros(0)))


def test_binned_cosine_representatives_past_lds(gpu):
    """Representatives of 1,025-5,000 peaks (the global-scratch path), mixed with
    ordinary ones in one call; one of them unsorted (the rank sort), one sharing
    bins with every member (runs of several peaks)."""
    rng = np.random.default_rng(41)
    clusters, reps = [], []
    for k, R in enumerate((300, 1025, 2048, 5000, 900, 1500)):
        base = np.sort(rng.uniform(100, 1900, 60))
        members = [{"m/z array": np.round(np.sort(base + rng.normal(0, 0.002, 60)), 5),
                    "intensity array": rng.lognormal(5, 1, 60)} for _ in range(3 + k)]
        clusters.append(members)
        rm = np.concatenate([np.repeat(base, 3) + rng.normal(0, 0.0005, 180), rng.uniform(100, 1990, R - 180)])
        rm = np.round(rm, 5)
        if k != 5:
            rm = np.sort(rm)  # cluster 5: an unsorted representative
        reps.append((rm, rng.lognormal(4, 1, len(rm))))
    csr = SpectraCSR.from_clusters(clusters)
    rep_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in reps])])
    rep_mz, rep_int = np.concatenate([r[0] for r in reps]), np.concatenate([r[1] for r in reps])
    got = _run(csr, rep_off, rep_mz, rep_int)
    assert np.all(got[2][:csr.n_clusters] == 0)
    _check(got, np_oracle.binned_cosine(csr, rep_off, rep_mz, rep_int), csr.n_clusters, csr.n_spectra)


# ---- the branches ordinary spectra never take (tests/binned_cosine_cases.py), against the
# reference's own results on them (tests/golden/binned_cosine_edges.npz)
@pytest.fixture(scope="module")
def edge_golden():
    import os

    from conftest import GOLDEN

    return np.load(os.path.join(GOLDEN, "binned_cosine_edges.npz"))


def _run_case(z, name):
    csr, rep_off, rep_mz, rep_int, s, want = cases.golden_case(z, name)
    got = _run(csr, rep_off, rep_mz, rep_int, s)
    _check(got, want, csr.n_clusters, csr.n_spectra)
    return got, want, csr


def test_binned_cosine_rep_on_edge(gpu, edge_golden):
    """Representative peaks on the rightmost edge of the pair's cut: shifted into the last
    bin (with and without a run of that bin, sorted or not, below and past the bucket
    table), and ordinary bins against a member that ends higher."""
    _run_case(edge_golden, "rep_on_edge")


def test_binned_cosine_high_mz(gpu, edge_golden):
    """Bins on both sides of 524,288, the end of the bucket table (m/z ~2,622.77), up to
    m/z 4,500: the binary-search tail of the run lookup, in both kernels."""
    _run_case(edge_golden, "high_mz")


def test_binned_cosine_chunk_runs(gpu, edge_golden):
    """Runs of one bin longer than a chunk, ending exactly at a chunk's last peak,
    filling a chunk, and closing a member of 64, 65 or 128 peaks."""
    _run_case(edge_golden, "chunk_runs")


def test_binned_cosine_sandwiched(gpu, edge_golden):
    """An invalid peak (above the cut, below the first edge, NaN) between two peaks of
    one bin, inside a chunk and across a chunk boundary: one sum, not two."""
    _run_case(edge_golden, "sandwiched")


def test_binned_cosine_many_deferred(gpu, edge_golden):
    """More deferred clusters than the global-scratch kernel has workgroups: every slice
    serves a second, shorter representative.  Twice on one DeviceBatch (the workspace is
    reused): the same bits."""
    csr, rep_off, rep_mz, rep_int, s, want = cases.golden_case(edge_golden, "many_deferred")
    assert int((np.diff(rep_off) > cases.RCAP).sum()) > cases.FALLBACK_BLOCKS
    b = engine.DeviceBatch.from_host(csr)
    dev = [_dev(rep_off), _dev(rep_mz), _dev(rep_int)]
    first = engine.binned_cosine(b, *dev, mz_space=s).to_host()
    second = engine.binned_cosine(b, *dev, mz_space=s).to_host()
    _check(first, want, csr.n_clusters, csr.n_spectra)
    _check(second, want, csr.n_clusters, csr.n_spectra)
    for x, y in zip(first, second):
        np.testing.assert_array_equal(x, y)


def test_binned_cosine_rcap_boundary(gpu, edge_golden):
    """One cluster with the first 511, 512 and 513 peaks of one representative: the last
    lengths of the LDS kernel and the first of the global-scratch kernel."""
    got, want, csr = _run_case(edge_golden, "rcap_boundary")
    n = csr.n_spectra // 3
    cos, wcos = got[0][:csr.n_spectra].reshape(3, n), want[0].reshape(3, n)
    for i, j in ((0, 1), (1, 2), (0, 2)):
        same = wcos[i] == wcos[j]
        np.testing.assert_array_equal(cos[i][same], cos[j][same])
        if want[1][i] == want[1][j]:
            assert got[1][i] == got[1][j]


@pytest.mark.parametrize("s", cases.SPACINGS)
def test_binned_cosine_mz_space(gpu, edge_golden, s):
    """Other bin widths: the edges, and the decimals of the on-edge rounding (8, 7, 7, 6),
    with an on-edge member and an on-edge representative built for each."""
    _run_case(edge_golden, f"mz_space_{s}")


def test_binned_cosine_nonfinite(gpu, edge_golden):
    """Infinite and NaN intensities as the reference's dense dot products treat them: an
    infinite bin inside the cut gives NaN unless the partner is all zero (0.0), past the
    cut it is dropped, and a finite square that overflows gives 0.0."""
    _run_case(edge_golden, "nonfinite")


def test_binned_cosine_unresolved_past_max_rep_peaks(gpu, edge_golden):
    """A representative longer than the caller's max_rep_peaks is reported unresolved
    (include/specpride.h); every other cluster of the call is scored."""
    csr, rep_off, rep_mz, rep_int, s, want = cases.golden_case(edge_golden, "unresolved")
    lens = np.diff(rep_off)
    b = engine.DeviceBatch.from_host(csr)
    cos, avg, st = engine.binned_cosine(b, _dev(rep_off), _dev(rep_mz), _dev(rep_int), mz_space=s,
                                        max_rep_peaks=cases.UNRESOLVED_MAX_REP).to_host()
    long = lens > cases.UNRESOLVED_MAX_REP
    assert long.sum() == 1 and (lens[~long] > cases.RCAP).sum() == 2
    assert np.all(st[:csr.n_clusters][long] == engine.STATUS_UNRESOLVED)
    keep = ~np.repeat(long, np.diff(csr.cluster_off))
    np.testing.assert_array_equal(st[:csr.n_clusters][~long], want[2][~long])
    np.testing.assert_allclose(cos[:csr.n_spectra][keep], want[0][keep], rtol=RTOL, atol=0, equal_nan=True)
    np.testing.assert_allclose(avg[:csr.n_clusters][~long], want[1][~long], rtol=RTOL, atol=0, equal_nan=True)
