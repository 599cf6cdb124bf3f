"""GPU parity of the explained b/y intensity (spx_by_fraction, engine.by_fraction and the
benchmark shims) against the numpy restatement of tests/by_fraction_cases.py.

Bar: statuses exact, every 0.0 the restatement decides exact, every other fraction within
1e-12 relative with NaN positions equal.  Both sides are quotients of two sums of at most
5,000 non-negative terms, each within n * 2^-53 = 5.6e-13 of the exact sum whatever the
order; test_by_fraction_inputs.py shows that no committed peak sits within 1e-9 relative of
a decision's edge, so which peaks count never hangs on a last bit."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import by_fraction_cases as cases
from specpride_amd import _lib, benchmark, engine

pytestmark = pytest.mark.gpu


def _params(overrides):
    p = _lib.default_by_params()
    for k, v in (overrides or {}).items():
        if len(k) == 1:
            p.aa_mass[ord(k) - ord("A")] = v
        else:
            setattr(p, k, v)
    return p


def _device_args(c, device):
    seqs = [p.encode("ascii") for p in c["peptides"]]
    seq_off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(b) for b in seqs], out=seq_off[1:])
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
    return (dev(c["mz"]), dev(c["inten"]), dev(c["seg_begin"]), dev(c["seg_end"]), dev(c["prec_mz"]),
            dev(c["charge"]), dev(np.frombuffer(b"".join(seqs), np.uint8).copy()), dev(seq_off))


def _run(name, device, **kw):
    c = cases.case(name)
    return engine.by_fraction(*_device_args(c, device), params=_params(c["params"]), **kw)


def _check(got, want, n):
    fraction, status = got
    wfraction, wstatus = want
    print("fraction", fraction[:n].tolist(), "expected", wfraction.tolist())
    np.testing.assert_array_equal(status[:n], wstatus)
    np.testing.assert_array_equal(np.isnan(fraction[:n]), np.isnan(wfraction))
    np.testing.assert_array_equal(fraction[:n] == 0.0, wfraction == 0.0)
    np.testing.assert_allclose(fraction[:n], wfraction, rtol=cases.RTOL, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", cases.NAMES)
def test_named_cases(gpu, name):
    want = cases.expect(name)
    _check(_run(name, gpu).to_host(), want, len(want[0]))


@pytest.mark.parametrize("key", list(cases.PARAM_SETS))
def test_params_move_the_result_as_the_restatement_says(gpu, key):
    want = cases.expect(f"params_{key}")
    got = _run(f"params_{key}", gpu).to_host()
    _check(got, want, len(want[0]))
    assert not np.array_equal(got[0][:len(want[0])], _run("fuzz0", gpu).to_host()[0][:len(want[0])])


def test_out_reuse_and_side_stream_give_identical_bits(gpu):
    base = [_run(n, gpu).to_host() for n in ("fuzz1", "unsorted_long")]
    n = len(base[0][0])
    out = engine.ByFractionResult(torch.full((n,), -1.0, dtype=torch.float64, device=gpu),
                                  torch.full((n,), -1, dtype=torch.int32, device=gpu))
    again = _run("fuzz1", gpu, out=out)
    assert again is out
    f, s = out.to_host()
    assert f.tobytes() == base[0][0].tobytes() and s.tobytes() == base[0][1].tobytes()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        res = [_run(nm, gpu, stream=side) for nm in ("fuzz1", "unsorted_long")]
    side.synchronize()
    for r, b in zip(res, base):
        f, s = r.to_host()
        assert f.tobytes() == b[0].tobytes() and s.tobytes() == b[1].tobytes()
    with pytest.raises(ValueError):
        _run("unsorted_long", gpu, out=engine.ByFractionResult(out.fraction[:1], out.status[:1]))


def test_no_segments_and_bad_arguments(gpu):
    e64 = torch.zeros(0, dtype=torch.float64, device=gpu)
    ei64 = torch.zeros(0, dtype=torch.int64, device=gpu)
    res = engine.by_fraction(e64, e64, ei64, ei64, e64, torch.zeros(0, dtype=torch.int32, device=gpu),
                             torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu))
    torch.cuda.synchronize()
    assert res.fraction.numel() == 1
    with pytest.raises(ValueError):
        engine.by_fraction(e64, e64, ei64, ei64, e64, torch.zeros(0, dtype=torch.int64, device=gpu),
                           torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu))
    L = _lib.lib()
    p = _lib.default_by_params()
    one = torch.zeros(2, dtype=torch.int64, device=gpu)
    assert L.spx_by_fraction(None, None, 0, one.data_ptr(), one.data_ptr(), -1, None, None, None, None, None, None,
                             None, None) == -1
    assert L.spx_by_fraction(None, None, 0, one.data_ptr(), one.data_ptr(), 1, None, None, None, one.data_ptr(),
                             None, None, None, None) == -1
    assert L.spx_by_fraction(None, None, 0, None, None, 0, None, None, None, None, None, None, None, None) == -1
    assert L.spx_by_fraction(None, None, 0, None, None, 0, None, None, None, None, ctypes.byref(p), None, None,
                             None) == 0


def test_shims_equal_the_restatement(gpu):
    c = cases.case("fuzz2")
    want = cases.expect("fuzz2")[0]
    spectra = [cases.Spectrum(c["mz"][b:e], c["inten"][b:e], p, int(z))
               for b, e, p, z in zip(c["seg_begin"], c["seg_end"], c["prec_mz"], c["charge"])]
    got = benchmark.fraction_of_by_batch(c["peptides"], c["prec_mz"], c["charge"], spectra)
    np.testing.assert_allclose(got, want, rtol=cases.RTOL, atol=0)
    one = benchmark.fraction_of_by(c["peptides"][3], c["prec_mz"][3], int(c["charge"][3]), spectra[3].mz,
                                   spectra[3].intensity)
    assert one == got[3]
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        assert benchmark.fraction_of_by("PEPTIDEX", 500.0, 2, spectra[0].mz, spectra[0].intensity) == 0.0
    assert err.getvalue() == "Invalid peptide sequence encountered\n"
    with pytest.raises(ValueError):
        benchmark.fraction_of_by("PEPTIDEK", 500.0, 2, [200.0, float("inf")], [1.0, 1.0])


def test_best_by_explained(gpu):
    clusters, peptides = cases.best_clusters()
    windices, wfractions = cases.best_expect()
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        indices, fractions = benchmark.best_by_explained(clusters, peptides)
    assert indices == windices
    for f, w in zip(fractions, wfractions):
        np.testing.assert_allclose(f, w, rtol=cases.RTOL, atol=0)
    assert err.getvalue().count("Invalid peptide") == len(clusters[5])


def test_cli_equals_the_batch_call(gpu, tmp_path):
    c = cases.case("fuzz3")
    titles = [f"cluster-{k // 3};mzspec:PXD000000:run{k}:scan:{100 + k}:{p}/{int(z)}"
              for k, (p, z) in enumerate(zip(c["peptides"], c["charge"]))]
    titles[4] = "cluster-1;mzspec:PXD000000:run4:scan:104"
    path = tmp_path / "clusters.mgf"
    with open(path, "w") as fh:
        for k, t in enumerate(titles):
            fh.write(f"BEGIN IONS\nTITLE={t}\nPEPMASS={float(c['prec_mz'][k])!r}\nCHARGE={int(c['charge'][k])}+\n")
            for m, i in zip(c["mz"][c["seg_begin"][k]:c["seg_end"][k]], c["inten"][c["seg_begin"][k]:c["seg_end"][k]]):
                fh.write(f"{float(m)!r} {float(i)!r}\n")
            fh.write("END IONS\n\n")
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        assert benchmark.main([str(path)]) == 0
    spectra = [cases.Spectrum(c["mz"][b:e], c["inten"][b:e], p, int(z))
               for b, e, p, z in zip(c["seg_begin"], c["seg_end"], c["prec_mz"], c["charge"])]
    with contextlib.redirect_stderr(io.StringIO()):
        want = benchmark.fraction_of_by_batch([p if k != 4 else "?" for k, p in enumerate(c["peptides"])],
                                              c["prec_mz"], c["charge"], spectra)
    assert out.getvalue().splitlines() == [f"{t}\t{float(f)!r}" for t, f in zip(titles, want)]
    assert want[4] == 0.0 and np.count_nonzero(want) >= 8
    assert err.getvalue() == "Invalid peptide sequence encountered\n"
