"""GPU parity of the cosine medoid (spx_cosine_medoid, engine.cosine_medoid) against
the oracle composition of tests/cosine_medoid_cases.py and the reference's own
average_cos_dist (tests/golden/cosine_medoid.npz).  Bar: rep and status exact on every
cluster (test_cosine_medoid_inputs.py shows that no committed cluster has a near-tie),
scores within 1e-12 relative with NaN positions equal."""
import contextlib
import io
import json
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest

import cosine_medoid_cases as cases
from conftest import GOLDEN, load_golden
from specpride_amd import benchmark, engine
from specpride_amd import most_similar_representative as msr
from specpride_amd.csr import SpectraCSR
from specpride_amd.mgf import read_mgf
from test_sharded_cli import write_records

pytestmark = pytest.mark.gpu


def _check(got, want, clusters):
    C, S = len(clusters), sum(len(c) for c in clusters)
    rep, score, status = got
    wrep, wscore, wstatus = want
    np.testing.assert_array_equal(status[:C], wstatus)
    np.testing.assert_array_equal(rep[:C], wrep)
    np.testing.assert_allclose(score[:S], wscore, rtol=cases.RTOL, atol=0, equal_nan=True)


def _run(clusters, **kw):
    batch = engine.DeviceBatch.from_host(cases.to_csr(clusters))
    return engine.cosine_medoid(batch, with_scores=True, **kw).to_host()


def test_reference_golden(gpu):
    z, csr = load_golden("cosine_medoid.npz")
    batch = engine.DeviceBatch.from_host(csr)
    rep, score, status = engine.cosine_medoid(batch, mz_space=float(z["mz_space"]), with_scores=True).to_host()
    np.testing.assert_array_equal(rep[:csr.n_clusters], z["rep"])
    np.testing.assert_allclose(score[:csr.n_spectra], z["score"], rtol=cases.RTOL, atol=0)
    assert np.all(status[:csr.n_clusters] == engine.STATUS_OK)
    # without scores: the same representatives
    rep2, none, _ = engine.cosine_medoid(batch, mz_space=float(z["mz_space"])).to_host()
    assert none is None
    np.testing.assert_array_equal(rep2[:csr.n_clusters], z["rep"])


@pytest.mark.parametrize("name", ["golden", "small", "duplicates", "cut", "order", "empty", "run_seams",
                                  "member_seams", "lds_runs", "long_spectrum"])
def test_named_cases(gpu, name):
    clusters = cases.clusters_of(name)
    _check(_run(clusters), cases.expect(name), clusters)


def test_exact_ties_go_to_the_first(gpu):
    """n = 2 and duplicated members tie bit for bit on the device too."""
    clusters = cases.clusters_of("small") + cases.clusters_of("duplicates")
    rep, score, _ = _run(clusters)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clusters])])
    assert score[off[1]] == score[off[1] + 1]                       # small[1]: n = 2
    d0, d1 = off[5], off[6]
    assert score[d0] == score[d0 + 3] == score[d0 + 5] and rep[5] == d0
    assert score[d1 + 1] == score[d1 + 4] and rep[6] == d1 + 1
    assert score[off[0]] == 1.0                                     # n = 1: a / sqrt(a * a)


@pytest.mark.parametrize("seed", range(cases.N_FUZZ))
def test_fuzz(gpu, seed):
    clusters = cases.clusters_of(f"fuzz{seed}")
    _check(_run(clusters), cases.expect(f"fuzz{seed}"), clusters)


def test_outside_the_limits_is_unresolved(gpu):
    """An m/z at or past COSINE_MEDOID_MAX_MZ, an infinite one, or a last m/z the
    reference cannot build edges from: SPX_UNRESOLVED and no index; the clusters next
    to them are untouched."""
    good = cases.clusters_of("small")[2]
    hi = engine.COSINE_MEDOID_MAX_MZ
    bad = [[(np.array([100.0, hi * 1.001]), np.array([1.0, 2.0])), good[0]],
           [(np.array([100.0, np.inf, 200.0]), np.array([1.0, 2.0, 3.0])), good[0]],
           [good[0], (np.array([100.0, np.nan]), np.array([1.0, 2.0]))],
           [good[0], (np.array([100.0, 0.001]), np.array([1.0, 2.0]))],
           [(np.array([100.0, 200.0]), np.array([np.inf, 2.0])), good[0]]]
    clusters = [good, *bad, good]
    rep, score, status = _run(clusters)
    assert list(status[:7]) == [0, 100, 100, 100, 100, 100, 0]
    assert np.all(rep[1:6] == -1) and np.isnan(score[3:13]).all()
    want = cases.expect("small")
    n0 = sum(len(c) for c in cases.clusters_of("small")[:2])
    assert rep[0] == want[0][2] - n0 and rep[6] - 13 == rep[0]
    np.testing.assert_allclose(score[:3], want[1][n0:n0 + 3], rtol=cases.RTOL, atol=0)
    # just inside the limit still resolves
    ok = [[(np.array([100.0, hi * 0.999]), np.array([1.0, 2.0])), (np.array([100.0, 300.0]), np.array([1.0, 2.0]))]]
    assert _run(ok)[2][0] == engine.STATUS_OK


def test_reuse_and_side_stream(gpu):
    import torch

    clusters = cases.clusters_of("golden") + cases.clusters_of("member_seams")[1:2]
    want = (np.concatenate([cases.expect("golden")[0], cases.expect("member_seams")[0][1:2] - 64 + 60]),
            np.concatenate([cases.expect("golden")[1], cases.expect("member_seams")[1][64:129]]),
            np.concatenate([cases.expect("golden")[2], cases.expect("member_seams")[2][1:2]]))
    batch = engine.DeviceBatch.from_host(cases.to_csr(clusters))
    out = engine.cosine_medoid(batch, with_scores=True)
    first = out.to_host()
    _check(first, want, clusters)
    ws = batch._bufs["cosine_medoid"].data_ptr()
    out.rep.fill_(-7)
    out.score.fill_(-7.0)
    again = engine.cosine_medoid(batch, out=out)
    assert again is out and batch._bufs["cosine_medoid"].data_ptr() == ws
    for a, b in zip(first, out.to_host()):
        np.testing.assert_array_equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = engine.cosine_medoid(batch, with_scores=True, stream=side)
    for a, b in zip(first, res.to_host()):
        np.testing.assert_array_equal(a, b)


def test_most_similar_by_cosine(gpu):
    clusters = cases.clusters_of("golden")
    objs = [[SimpleNamespace(mz=m, intensity=i) for m, i in cl] for cl in clusters]
    idx, scores = benchmark.most_similar_by_cosine(objs)
    z, csr = load_golden("cosine_medoid.npz")
    assert idx == list(z["rep"] - csr.cluster_off[:-1])
    np.testing.assert_allclose(np.concatenate(scores), z["score"], rtol=cases.RTOL, atol=0)
    assert benchmark.most_similar_by_cosine([[], objs[0]])[0] == [-1, 0]
    with pytest.raises(IndexError):
        benchmark.most_similar_by_cosine([objs[1] + [SimpleNamespace(mz=np.zeros(0), intensity=np.zeros(0))]])


# ------------------------------------------------------------------------ CLI
@pytest.fixture(scope="module")
def rccl_world1():
    import torch.distributed as dist

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def golden_mgf(tmp_path_factory):
    """The golden clusters as a clustered MGF, the members of different clusters interleaved."""
    clusters = cases.clusters_of("golden")
    csr = cases.to_csr(clusters)
    S = csr.n_spectra
    csr = SpectraCSR(csr.cluster_off, csr.spec_off, csr.mz, csr.inten, 500.0 + 0.25 * np.arange(S),
                     np.full(S, 2, np.int32), 10.0 * np.arange(S))
    owner = np.repeat(np.arange(csr.n_clusters), np.diff(csr.cluster_off))
    titles = [f"cl{owner[s]};mzspec:PXDSYN:synthetic:scan:{s}" for s in range(csr.n_spectra)]
    order = np.arange(csr.n_spectra)
    order[10:20] = order[10:20][np.random.default_rng(2).permutation(10)]  # split runs (the reference's scan)
    path = str(tmp_path_factory.mktemp("cosmed") / "golden.mgf")
    write_records(path, csr, order, titles)
    return path


def _helper_choice(path):
    """Titles the oracle chooses: the reference's cluster scan, then the helper."""
    spectra = read_mgf(path)
    names = [sp["params"]["title"].split(";")[0] for sp in spectra]
    titles = []
    for _cl, members in msr._first_runs(names):
        if members:
            cl = [(np.asarray(spectra[i]["m/z array"], np.float64), np.asarray(spectra[i]["intensity array"], np.float64))
                  for i in members]
            titles.append(spectra[members[cases.scores_and_rep(cl)[1]]]["params"]["title"])
    return titles


def _main(argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        msr.main(argv)
    return out.getvalue()


@pytest.mark.parametrize("which", ["golden", "noncontiguous"])
def test_cli_cosine_native_dict_device_sharded_identical(gpu, rccl_world1, golden_mgf, tmp_path, which, monkeypatch):
    from specpride_amd import device_ingest, mgf_native, sharded_cli

    src = golden_mgf if which == "golden" else os.path.join(GOLDEN, "medoid_noncontiguous.mgf")
    native, dicts, device, sharded = (tmp_path / f"{k}.mgf" for k in "ndvs")
    monkeypatch.delenv(device_ingest.ENV, raising=False)
    out_n = _main(["-i", src, "-o", str(native), "-m", "cosine"])
    want = native.read_bytes()
    assert [s["params"]["title"] for s in read_mgf(str(native))] == _helper_choice(src)
    out_s = io.StringIO()
    with contextlib.redirect_stdout(out_s):
        assert sharded_cli.medoid(src, str(sharded), device=gpu, compute=msr.cosine_compute) is None
    loads = []
    real_load = device_ingest.load
    with monkeypatch.context() as m:
        m.setenv(device_ingest.ENV, "1")
        m.setattr(device_ingest, "load", lambda *a, **k: loads.append(a) or real_load(*a, **k))
        out_v = _main(["-i", src, "-o", str(device), "-m", "cosine"])
    assert len(loads) == 1, "the device-ingest path did not run"
    seen = []
    real_read = msr.read_mgf
    monkeypatch.setattr(mgf_native, "parse_general", lambda *a, **k: None)
    monkeypatch.setattr(msr, "read_mgf", lambda path: seen.append(path) or real_read(path))
    out_d = _main(["-i", src, "-o", str(dicts), "-m", "cosine"])
    assert seen == [src], "the dict path did not run"
    assert out_n == out_d == out_v == out_s.getvalue()
    assert dicts.read_bytes() == want
    assert device.read_bytes() == want
    assert sharded.read_bytes() == want


def test_cli_default_method_is_unchanged(gpu, tmp_path):
    """Without -m (and with -m xcorr) the CLI picks the reference's xcorr medoids
    (tests/golden/medoid_noncontiguous.json) and writes the same bytes."""
    src = os.path.join(GOLDEN, "medoid_noncontiguous.mgf")
    plain, xcorr = tmp_path / "p.mgf", tmp_path / "x.mgf"
    assert _main(["-i", src, "-o", str(plain)]) == _main(["-i", src, "-o", str(xcorr), "-m", "xcorr"])
    gold = json.load(open(os.path.join(GOLDEN, "medoid_noncontiguous.json")))
    assert [s["params"]["title"] for s in read_mgf(str(plain))] == gold["titles"]
    assert plain.read_bytes() == xcorr.read_bytes()


def test_cli_unknown_method_exits_2(gpu, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        msr.main(["-i", os.path.join(GOLDEN, "medoid_noncontiguous.mgf"), "-o", str(tmp_path / "o.mgf"), "-m", "bogus"])
    assert e.value.code == 2 and not (tmp_path / "o.mgf").exists()
    assert capsys.readouterr().out == "most_similar_representative.py -i <inputfile> -o <outputfile>\n"
