"""CPU checks of the explained b/y intensity's test inputs (tests/by_fraction_cases.py) and
of the benchmark shims' host side: hand values, the restatement against an order-free
brute force on every committed case, the condition that keeps the GPU comparison honest
(no case leans on a last-bit decision), and the peptide parsing with the device call
replaced."""
import ctypes
import types

import numpy as np
import pytest

import by_fraction_cases as cases
from specpride_amd import _lib, benchmark, engine

ALL = cases.NAMES + [f"params_{k}" for k in cases.PARAM_SETS]


def test_hand_values():
    aa, const = cases.params_of()
    fr = cases.fragments("WK", 2, aa, const)
    assert len(fr) == 2 and abs(fr[0] - 187.08658646677) < 1e-9 and abs(fr[1] - 147.11280115047) < 1e-9
    assert (fr[0], fr[1]) == pytest.approx(cases.WK[1:], abs=1e-9)
    # b1 = W + proton, y1 = K + water + proton, by hand
    assert abs(fr[0] - (186.07931 + 1.00727646677)) < 1e-9
    assert abs(fr[1] - (128.09496 + 2 * 1.00782503207 + 15.99491461956 + 1.00727646677)) < 1e-9
    # exactly those two peaks (3 + 5) and one unrelated peak (8): 8 / 16
    assert cases.restate("WK", 400.0, 2, [147.11280115047, 187.08658646677, 300.0], [3.0, 5.0, 8.0]) == (0.5, 0)
    # charge 3 adds the doubly charged pair, (m + 2 p) / 2
    fr3 = cases.fragments("WK", 3, aa, const)
    assert len(fr3) == 4 and abs(fr3[2] - (186.07931 + 2 * 1.00727646677) / 2) < 1e-9


def test_default_params_are_the_restatement_s():
    p = _lib.default_by_params()
    assert ctypes.sizeof(p) == 33 * 8
    aa, const = cases.params_of()
    for k in range(26):
        letter = chr(ord("A") + k)
        assert p.aa_mass[k] == aa[letter] if letter in aa else np.isnan(p.aa_mass[k])
    assert sorted(aa) == sorted(cases.RESIDUES) == sorted(benchmark.VALID_RESIDUES)
    for k, v in const.items():
        assert getattr(p, k) == v
    assert (engine.BY_MAX_SEQ, engine.BY_MAX_CHARGE) == (cases.MAX_SEQ, cases.MAX_CHARGE)
    assert "spx_by_fraction" in _lib.EXPORTED


@pytest.mark.parametrize("name", ALL)
def test_restatement_equals_the_order_free_formulation(name):
    """The kept and the annotated peaks of the libraries' sorted loops are those of a
    formulation with no sort: rule 2's order (m/z, then input index) is all that matters."""
    c = cases.case(name)
    built = 0
    for _, seq, prec, z, mz, inten in cases.segments(c):
        got = cases.brute(seq, prec, z, mz, inten, c["params"])
        frac, status, kept, annotated = cases.restate(seq, prec, z, mz, inten, c["params"], detail=True)
        if got is None:
            assert status == cases.STATUS_UNRESOLVED or frac == 0.0
            continue
        built += 1
        np.testing.assert_array_equal(kept, got[0])
        np.testing.assert_array_equal(annotated, got[1])
    assert built or name in ("bad_sequences",)


def _edges(c):
    """Per valid segment: the smallest relative distance of a peak to a window edge, a range
    end (exact hits on the ends excepted) or a precursor window edge."""
    aa, const = cases.params_of(c["params"])
    t = const["tol_ppm"] * 1e-6
    for _, seq, prec, z, mz, inten in cases.segments(c):
        if cases.brute(seq, prec, z, mz, inten, c["params"]) is None or not len(mz):
            continue
        centres = list(cases.fragments(seq, z, aa, const)) + (cases.precursor_mzs(prec, z, const) if z > 0 else [])
        edge = np.array([f * s for f in centres for s in (1 - t, 1 + t)] + [const["min_mz"], const["max_mz"]])
        d = np.abs(mz[:, None] - edge[None, :]) / np.abs(edge[None, :])
        d[(mz[:, None] == edge[None, :]) & (np.arange(len(edge)) >= len(edge) - 2)[None, :]] = np.inf
        yield float(d.min())


@pytest.mark.parametrize("name", ALL)
def test_no_case_leans_on_a_last_bit_decision(name):
    """No peak within 1e-9 relative of a window edge, a range end or a precursor window edge,
    apart from the exact range ends 100.0 and 1400.0: which side a peak is on never hangs
    on the rounding of the ppm expression."""
    for d in _edges(cases.case(name)):
        assert d > 1e-9


def test_range_ends_are_hit_exactly():
    c = cases.case("range_ends")
    assert 100.0 in c["mz"] and 1400.0 in c["mz"] and 99.999 in c["mz"] and 1400.001 in c["mz"]
    frac, _, kept, _ = cases.restate(c["peptides"][0], 700.0, 2, c["mz"][:5], c["inten"][:5], detail=True)
    np.testing.assert_array_equal(kept, [1, 2, 3])
    assert frac == 2.0 / 7.0


def test_cases_cover_what_they_claim():
    f, s = cases.expect("window")
    np.testing.assert_array_equal(f[:8] > 0, [True, False] * 4)
    assert f[8] == 4.0 / 15.0  # both inside ones share b1's window: the stronger one
    f, _ = cases.expect("shared_tied")
    assert list(f) == [9.0 / 10.0, 9.0 / 16.0, 7.0 / 16.0, 7.0 / 16.0]
    f, _ = cases.expect("tie_union")
    assert list(f) == [0.5, 0.5]  # {P1, P2} of 16; the other tie-break would give 0.25
    c = cases.case("precursor")
    _, _, kept, _ = cases.restate(c["peptides"][0], 300.0, 3, c["mz"][:9], c["inten"][:9], detail=True)
    np.testing.assert_array_equal(kept, [0, 1, 5, 8])  # r3, r2, r1 and the two within 49 ppm are gone
    f, s = cases.expect("nonfinite")
    assert list(s) == [0] * 6 + [100] * 5 + [0]
    assert f[0] == 0.0 and f[1] == 0.25 and f[2] == 0.0 and np.isnan(f[3]) and f[4] == 0.0 and np.isnan(f[5])
    f, s = cases.expect("bad_sequences")
    assert np.all(s == 0) and np.all(f[:12] == 0.0) and f[12] == 0.25 and f[13] == 0.0
    f, s = cases.expect("limits")
    assert list(s) == [100, 0, 100, 100, 0]
    c = cases.case("unsorted_long")
    sizes = (c["seg_end"] - c["seg_begin"]).tolist()
    assert sizes[1:3] == [65, 5000] and 2000 < sizes[3] <= 3000
    srt = [bool(np.all(np.diff(c["mz"][b:e]) >= 0)) for b, e in zip(c["seg_begin"], c["seg_end"])]
    assert srt == [False, True, True, False]
    aa, const = cases.params_of()
    c = cases.case("seams")
    counts = [len(cases.fragments(p, int(z), aa, const)) for p, z in zip(c["peptides"], c["charge"])]
    assert counts == [2, 62, 64, 66, 126, 128, 130, 64, 2] and len(counts) % 4
    for name in cases.NAMES:  # value cases keep intensities non-negative
        assert not np.any(cases.case(name)["inten"] < 0)
    for k, ov in cases.PARAM_SETS.items():  # changed parameters move the result
        assert not np.array_equal(cases.expect(f"params_{k}")[0], cases.expect("fuzz0")[0]), ov


def test_best_clusters_have_no_near_ties():
    clusters, peptides = cases.best_clusters()
    indices, fractions = cases.best_expect()
    assert indices[2] == -1 and indices[5] == 0 and len(clusters[3]) == 10
    for cl, f, best in zip(clusters, fractions, indices):
        for k, s in enumerate(cl):
            if k == best:
                continue
            twin = np.array_equal(s.mz, cl[best].mz) and np.array_equal(s.intensity, cl[best].intensity)
            assert (twin and f[k] == f[best] and k > best) or f[k] < f[best] * (1 - 1e-9) or f[best] == 0.0
    assert fractions[3][indices[3]] == fractions[3][9] and indices[3] < 9  # the duplicate loses to the first


# ------------------------------------------------------------------ the shims' host side
class _Fake:
    """engine.by_fraction on the host: the restatement over the tensors it is handed."""

    def __init__(self):
        self.calls = []

    def __call__(self, mz, inten, seg_begin, seg_end, prec_mz, charge, seq, seq_off, params=None, out=None,
                 stream=None):
        a = [t.cpu().numpy() for t in (mz, inten, seg_begin, seg_end, prec_mz, charge, seq, seq_off)]
        peptides = [bytes(a[6][a[7][i]:a[7][i + 1]]).decode("ascii") for i in range(len(a[2]))]
        self.calls.append(peptides)
        res = [cases.restate(p, float(a[4][i]), int(a[5][i]), a[0][a[2][i]:a[3][i]], a[1][a[2][i]:a[3][i]])
               for i, p in enumerate(peptides)]
        fraction = np.array([r[0] for r in res] or [0.0])
        status = np.array([r[1] for r in res] or [0], np.int32)
        return types.SimpleNamespace(fraction=fraction, status=status, to_host=lambda: (fraction, status))


def test_peptide_of_title():
    assert benchmark.peptide_of_title("cluster-3;mzspec:PXD004732:01650b_BC2:scan:17555:VLHPLEGAVVIIFK/2") == \
        "VLHPLEGAVVIIFK"
    assert benchmark.peptide_of_title("cluster-3;mzspec:PXD004732:01650b_BC2:scan:17555") == "175"
    assert benchmark.peptide_of_title("") == ""
    assert benchmark.fast_valid("VLHPLEGAVVIIFK") and benchmark.fast_valid("")
    for bad in ("175", "PEPXIDE", "peptide", "_(ac)PEPTIDEK_", "PEPTIDEB", "PEP TIDE"):
        assert not benchmark.fast_valid(bad)


def test_fraction_of_by_shim(monkeypatch, capsys):
    fake = _Fake()
    monkeypatch.setattr(engine, "by_fraction", fake)
    y1 = 147.11280115047
    assert benchmark.fraction_of_by("WK", 400.0, 2, [y1, 300.0], [1.0, 3.0], device="cpu") == 0.25
    assert capsys.readouterr().err == ""
    # an invalid peptide: 0.0 and the reference's message; the device sees one byte that is no residue
    assert benchmark.fraction_of_by("_(ac)WK_", 400.0, 2, [y1, 300.0], [1.0, 3.0], device="cpu") == 0.0
    assert capsys.readouterr().err == "Invalid peptide sequence encountered\n"
    assert fake.calls == [["WK"], ["?"]]
    assert benchmark.fraction_of_by("wké", 400.0, 2, [y1, 300.0], [1.0, 3.0], device="cpu") == 0.0
    capsys.readouterr()
    with pytest.raises(ValueError):
        benchmark.fraction_of_by("WK", 400.0, 2, [y1, float("nan")], [1.0, 3.0], device="cpu")
    with pytest.raises(ValueError):
        benchmark.fraction_of_by("WK", float("inf"), 2, [y1, 300.0], [1.0, 3.0], device="cpu")
    with pytest.raises(ValueError):
        benchmark.fraction_of_by("WK", 400.0, 2, [y1, 300.0], [1.0], device="cpu")
    # invalid and a non-finite m/z: the reference returns before it looks at the spectrum
    assert benchmark.fraction_of_by("WX", 400.0, 2, [y1, float("nan")], [1.0, 3.0], device="cpu") == 0.0


def test_fraction_of_by_batch_shim(monkeypatch, capsys):
    fake = _Fake()
    monkeypatch.setattr(engine, "by_fraction", fake)
    y1 = 147.11280115047
    sp = [types.SimpleNamespace(mz=np.array([y1, 300.0]), intensity=np.array([1.0, 3.0])),
          types.SimpleNamespace(mz=np.zeros(0), intensity=np.zeros(0)),
          types.SimpleNamespace(mz=np.array([y1, 300.0]), intensity=np.array([1.0, 1.0]))]
    got = benchmark.fraction_of_by_batch(["WK", "WK", "W1"], [400.0] * 3, [2, 2, 2], sp, device="cpu")
    np.testing.assert_array_equal(got, [0.25, 0.0, 0.0])
    assert len(fake.calls) == 1 and fake.calls[0] == ["WK", "WK", "?"]
    assert capsys.readouterr().err.count("Invalid peptide sequence encountered") == 1
    with pytest.raises(ValueError):
        benchmark.fraction_of_by_batch(["WK"], [400.0] * 3, [2, 2, 2], sp, device="cpu")
    assert len(benchmark.fraction_of_by_batch([], [], [], [], device="cpu")) == 0


def test_cli_shim(monkeypatch, capsys, tmp_path):
    fake = _Fake()
    monkeypatch.setattr(engine, "by_fraction", fake)
    y1 = 147.11280115047
    titles = ["cluster-1;mzspec:PXD1:run:scan:7:WK/2", "cluster-1;mzspec:PXD1:run:scan:8", "cluster-2;x:WK/3"]
    path = tmp_path / "in.mgf"
    with open(path, "w") as fh:
        for t, z in zip(titles, (2, 2, 3)):
            fh.write(f"BEGIN IONS\nTITLE={t}\nPEPMASS=400.0\nCHARGE={z}+\n{y1!r} 1.0\n300.0 3.0\nEND IONS\n\n")
    assert benchmark.main([str(path)], device="cpu") == 0
    out, err = capsys.readouterr()
    assert out.splitlines() == [f"{titles[0]}\t0.25", f"{titles[1]}\t0.0", f"{titles[2]}\t0.25"]
    assert err == "Invalid peptide sequence encountered\n"
    assert fake.calls == [["WK", "?", "WK"]]
    assert benchmark.main([], device="cpu") == 2
