"""Device-side MGF ingest (specpride_amd/device_ingest.py, csrc/mgf_parse.hip)
against its oracle, the host parser ``mgf_native.parse_ranges`` (pinned to Python
float() and the Python readers by tests/test_mgf_native.py): bit-identical
arrays for the same records in the same order, or the same whole-file fallback;
no re-parse flag on canonical records; the three CLIs byte-identical with
``SPX_DEVICE_INGEST=1``.
"""
import contextlib
import glob
import io
import os
import re
from decimal import Decimal, getcontext

import numpy as np
import pytest

from conftest import GOLDEN
from specpride_amd import average_spectrum_clustering as asc
from specpride_amd import binning, device_ingest, mgf_native
from specpride_amd import most_similar_representative as msr
from test_sharded_cli import synthetic_mgf

pytestmark = pytest.mark.gpu

OK, REPARSE = device_ingest.OK, device_ingest.REPARSE
TILE = 1024  # kMgfTile; the kernel's wave and block are 64 and 256
CANONICAL = ["bin_mean_cli_in.mgf", "best_spectrum_in.mgf", "medoid_noncontiguous.mgf", "bin_mean_cli_out.mgf"]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _host(path, begin, end, general):
    try:
        return mgf_native.parse_ranges(str(path), begin, end, general)
    except ValueError as e:
        assert "fallback" in str(e)
        return None


def _assert_equal(got, want, general, what=""):
    """Device result == parse_ranges, or both report the fallback."""
    if want is None:
        assert got is None, f"{what}: the host falls back, the device path does not"
        return
    assert got is not None, f"{what}: the device path falls back, the host does not"
    np.testing.assert_array_equal(got["host_spec_off"], want["spec_off"], err_msg=what)
    np.testing.assert_array_equal(got["spec_off"].cpu().numpy(), want["spec_off"], err_msg=what)
    np.testing.assert_array_equal(_bits(got["mz"].cpu().numpy()), _bits(want["mz"]), err_msg=what)
    np.testing.assert_array_equal(_bits(got["inten"].cpu().numpy()), _bits(want["inten"]), err_msg=what)
    hp, hc = want["has_prec"], want["has_charge"]
    np.testing.assert_array_equal((got["flags"] & 1) != 0, hp, err_msg=what)
    np.testing.assert_array_equal((got["flags"] & 2) != 0, hc, err_msg=what)
    prec, charge = got["prec_mz"].cpu().numpy(), got["charge"].cpu().numpy()
    if general:
        np.testing.assert_array_equal((got["flags"] & 4) != 0, want["has_rt"], err_msg=what)
        np.testing.assert_array_equal((got["flags"] & 8) != 0, want["has_title"], err_msg=what)
        np.testing.assert_array_equal(_bits(got["rt"].cpu().numpy()), _bits(want["rt"]), err_msg=what)
    else:
        # the binning parser carries PEPMASS / CHARGE over from the record it parsed
        # before when a record has none: the value is no property of the record
        prec, charge = prec[hp], charge[hc]
        assert np.isnan(got["rt"].cpu().numpy()).all()
    np.testing.assert_array_equal(_bits(prec), _bits(want["prec_mz"][hp] if not general else want["prec_mz"]),
                                  err_msg=what)
    np.testing.assert_array_equal(charge, (want["charge"][hc] if not general else want["charge"]).astype(np.int32),
                                  err_msg=what)


def _both(path, X, order, general, gpu, what="", fallback_ok=False):
    """parse_records (patched) vs parse_ranges over X's records in `order`; returns
    the kernel's own statuses (None if the index is empty)."""
    b, e, n = X["begin"][order], X["end"][order], X["npk"][order]
    raw = device_ingest.parse_records(str(path), b, e, n, general, gpu, patch=False)
    got = device_ingest.parse_records(str(path), b, e, n, general, gpu,
                                      title_of=lambda r: X["titles"][order[r]])
    want = _host(path, b, e, general)
    assert want is not None or fallback_ok, f"{what}: the host parser falls back on this input"
    _assert_equal(got, want, general, what)
    return raw["status"]


# ------------------------------------------------------------------ numbers
def _tokens():
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(50, 3000, 30000), rng.lognormal(3, 3, 30000), 10.0 ** rng.uniform(-20, 25, 30000)])
    vals = [f"{v:.5f}" for v in x[:10000]] + [f"{v:.2f}" for v in x[30000:36000]]  # short decimals
    vals += [repr(float(v)) for v in x]
    vals += [f"{v:.19g}" for v in x[:14000]]
    vals += [f"{v:.18e}" for v in x[20000:24000]]
    getcontext().prec = 40
    for v in x[:4000]:  # decimals halfway between adjacent doubles and a hair off them
        a = float(v)
        mid = (Decimal(a) + Decimal(float(np.nextafter(a, np.inf)))) / 2
        for d in (mid, mid.next_plus(), mid.next_minus()):
            vals.append(format(d.quantize(Decimal(1).scaleb(-17)) if abs(d) < 1e3 else d, "f")[:21])
    vals += ["0", "0.0", "-0.0", "123456789012345678901234.5", "1e300", "2.5e-310", "1" * 25, "9007199254740993",
             "9007199254740992.5", "18446744073709551615", "0.1", "-17.25", "0.000000000000000000000000001",
             "1234567890123456789.12345678", "0.0000000000000000000000000001", "00012.50", "7."]
    return vals


def _canonical(tok):
    """<dec> = digits[.digits], <= 19 significant and <= 27 fraction digits."""
    if not re.fullmatch(r"[0-9]+(\.[0-9]+)?", tok):
        return False
    whole, _, frac = tok.partition(".")
    return len((whole + frac).lstrip("0")) <= 19 and len(frac) <= 27


def test_numbers_equal_python_float(gpu, tmp_path):
    """~130k tokens as peak intensities: every value of an OK record equals Python
    float() bit for bit, the patched arrays equal parse_ranges, and a record whose
    tokens are all canonical is never flagged."""
    vals = _tokens()
    assert len(vals) > 120000
    vals.sort(key=lambda t: not _canonical(t))  # canonical tokens first: whole records of them
    per = 500
    path = tmp_path / "floats.mgf"
    with open(path, "w") as fh:
        for i in range(0, len(vals), per):
            fh.write(f"BEGIN IONS\nTITLE=c;s{i}\nPEPMASS=500.0\nCHARGE=2+\n")
            fh.writelines(f"{1 + i % 7} {v}\n" for v in vals[i:i + per])
            fh.write("END IONS\n")
    X = mgf_native.index(str(path), True)
    R = len(X["begin"])
    assert R == (len(vals) + per - 1) // per
    status = _both(path, X, np.arange(R), True, gpu)
    got = device_ingest.parse_records(str(path), X["begin"], X["end"], X["npk"], True, gpu, patch=False)
    inten = got["inten"].cpu().numpy()
    want = np.array([float(v) for v in vals])
    clean = np.array([all(_canonical(t) for t in vals[i:i + per]) for i in range(0, len(vals), per)])
    assert clean.sum() > 100 and (~clean).sum() > 20
    assert not status[clean].any(), f"canonical records flagged: {np.flatnonzero(status[clean] != OK)[:5]}"
    ok = np.repeat(status == OK, np.diff(got["host_spec_off"]))
    bad = np.flatnonzero(ok & (_bits(inten) != _bits(want)))
    assert len(bad) == 0, [(vals[i], inten[i], want[i]) for i in bad[:5]]


# ------------------------------------------------------------------ goldens
GOLDEN_MGF = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "*.mgf")))


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("name", GOLDEN_MGF)
def test_goldens_equal_parse_ranges(gpu, name, general):
    path = os.path.join(GOLDEN, name)
    X = mgf_native.index(path, general)
    order = np.random.default_rng(3).permutation(len(X["begin"]))
    status = _both(path, X, order, general, gpu, name, fallback_ok=True)
    accepted = _host(path, X["begin"], X["end"], general) is not None
    if name in CANONICAL:
        # bin_mean_cli_out.mgf has no "id;usi" titles: the binning parser falls back on it
        assert accepted == (general or name != "bin_mean_cli_out.mgf")
        if accepted:
            assert len(status) and not status.any()
    if name == "bin_mean_cli_nonfinite_in.mgf":
        text = open(path, "rb").read()
        exotic = np.array([re.search(rb"(?i)nan|inf|1e999", text[X["begin"][r]:X["end"][r]]) is not None
                           for r in order])
        assert exotic.any() and (status[exotic] == REPARSE).all()


# ------------------------------------------------------------------ shapes
def _record(k, npk, rng, title=None, pad=0):
    lines = ["BEGIN IONS", f"TITLE={title or f'cl{k % 5};scan:{k}'}", f"PEPMASS={400 + k}.{k % 97:02d}", "CHARGE=2+",
             f"RTINSECONDS={k}.5"]
    if pad:  # a line of exactly `pad` characters
        assert pad >= 5
        lines.append("NOTE=" + "x" * (pad - 5))
    mz = np.sort(rng.uniform(100, 2000, npk))
    it = rng.lognormal(3, 2, npk)
    lines += [f"{a:.5f} {b!r}" if i % 3 else f"{a:.4f} {b:.2f}" for i, (a, b) in enumerate(zip(mz, it.tolist()))]
    return lines + ["END IONS", ""]


def _write(path, records, eol, final=True):
    text = eol.join(eol.join(r) for r in records) + eol
    if not final:
        text = text.rstrip("\r\n")
    path.write_bytes(text.encode())
    return text


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 5000, 2, 0, 1]


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("eol", ["\n", "\r\n", "\r"], ids=["lf", "crlf", "cr"])
def test_peak_counts_and_line_ends(gpu, tmp_path, eol, general):
    """0 and 1 peak lines, counts around the wave (64), the block (256) and the tile
    (1,024), one record of 5,000 peaks; LF, CRLF and CR files; non-contiguous
    clusters (destination order != file order); the last record runs to EOF."""
    rng = np.random.default_rng(7)
    path = tmp_path / "shapes.mgf"
    _write(path, [_record(k, n, rng) for k, n in enumerate(SIZES)], eol)
    X = mgf_native.index(str(path), general)
    np.testing.assert_array_equal(X["npk"], SIZES)
    assert X["end"][-1] == os.path.getsize(path)
    ids, sizes, order, n_used, off = device_ingest.plan(X["titles"], X["npk"], mgf_native.GROUP_BINNING)
    assert not np.array_equal(order, np.arange(len(SIZES)))
    status = _both(path, X, order, general, gpu)
    assert not status.any()


@pytest.mark.parametrize("general", [False, True])
def test_no_final_terminator(gpu, tmp_path, general):
    """The file ends inside its last line ("END IONS" + EOF).  Parsed last, the
    record is canonical; parsed before another, the host parser reads its last line
    and the next record's first as one, and both sides must agree on that too."""
    rng = np.random.default_rng(8)
    path = tmp_path / "open.mgf"
    _write(path, [_record(k, n, rng) for k, n in enumerate([5, 70, 3])], "\n", final=False)
    assert open(path, "rb").read().endswith(b"END IONS")
    X = mgf_native.index(str(path), general)
    assert len(X["begin"]) == 3
    assert not _both(path, X, np.arange(3), general, gpu).any()
    _both(path, X, np.array([2, 0, 1]), general, gpu, fallback_ok=True)


@pytest.mark.parametrize("eol", ["\r\n", "\r"], ids=["crlf", "cr"])
def test_line_ends_at_tile_boundaries(gpu, tmp_path, eol):
    """A "\\r\\n" pair split exactly across each tile boundary of a record (the '\\r'
    is a tile's last byte) and a lone '\\r' line end there, for both grammars' record
    starts; records whose length is one less than, equal to and one more than a
    multiple of the tile.  A NOTE= line (ignored by both parsers) shifts the peaks."""
    begin_line = len("BEGIN IONS" + eol)  # a binning record starts at its TITLE= line
    records, aimed = [], []
    for k in range(21):
        plain = eol.join(_record(k, 200, np.random.default_rng(100 + k)))
        if k < 18:
            shift = begin_line * (k % 2)
            boundary = TILE * (1 + (k // 2) % 3)
            q = plain.rindex("\r", 0, shift + boundary - 8)
            add = shift + boundary - 1 - q
            aimed.append((k % 2 == 0, boundary))
        else:
            add = ((k - 19) - (len(plain) + len(eol))) % TILE
            add += TILE if add < 8 else 0
        records.append(_record(k, 200, np.random.default_rng(100 + k), pad=add - len(eol)))
    path = tmp_path / "tiles.mgf"
    text = _write(path, records, eol).encode()
    for general in (False, True):
        X = mgf_native.index(str(path), general)
        assert len(X["begin"]) == 21
        for k, (for_general, boundary) in enumerate(aimed):
            if for_general == general:
                at = int(X["begin"][k]) + boundary
                assert text[at - 1:at] == b"\r" and (text[at:at + 1] == b"\n") == (eol == "\r\n"), (k, general)
        if general:
            np.testing.assert_array_equal((X["end"] - X["begin"])[18:] % TILE, [TILE - 1, 0, 1])
        assert not _both(path, X, np.arange(21)[::-1].copy(), general, gpu).any()


@pytest.mark.parametrize("general", [False, True])
def test_tampered_peak_count_is_flagged_not_overrun(gpu, tmp_path, general):
    """An index peak count smaller or larger than the record's peak lines: the
    record is flagged, its neighbours' slots are untouched, and the patched parse
    refuses (the index and the parser disagree)."""
    rng = np.random.default_rng(10)
    path = tmp_path / "tamper.mgf"
    _write(path, [_record(k, 40, rng) for k in range(5)], "\n")
    X = mgf_native.index(str(path), general)
    want = _host(path, X["begin"], X["end"], general)
    npk = X["npk"].copy()
    npk[1] -= 7
    npk[3] += 7
    raw = device_ingest.parse_records(str(path), X["begin"], X["end"], npk, general, gpu, patch=False)
    np.testing.assert_array_equal(raw["status"], [OK, REPARSE, OK, REPARSE, OK])
    so, mz = raw["host_spec_off"], raw["mz"].cpu().numpy()
    for r in (0, 2, 4):
        np.testing.assert_array_equal(_bits(mz[so[r]:so[r + 1]]),
                                      _bits(want["mz"][want["spec_off"][r]:want["spec_off"][r + 1]]))
    assert device_ingest.parse_records(str(path), X["begin"], X["end"], npk, general, gpu) is None


def test_bad_ranges_are_flagged_or_rejected(gpu, tmp_path):
    """Ranges outside the text or slots outside the peak arrays are flagged per record
    without a read; sizes the host can check are SPX_EINVAL without a launch."""
    import torch

    from specpride_amd import _lib

    path = tmp_path / "r.mgf"
    _write(path, [_record(k, 10, np.random.default_rng(k)) for k in range(3)], "\n")
    X = mgf_native.index(str(path), True)
    size = os.path.getsize(path)
    begin, end = X["begin"].copy(), X["end"].copy()
    begin[0], end[2] = -5, size + 100
    raw = device_ingest.parse_records(str(path), begin, end, X["npk"], True, gpu, patch=False)
    np.testing.assert_array_equal(raw["status"], [REPARSE, OK, REPARSE])
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.int64, device=gpu)
    p = t.data_ptr()
    assert L.spx_parse_mgf_text(p, -1, p, p, p, 1, 1, 0, p, p, p, p, p, p, p, None) == -1
    assert L.spx_parse_mgf_text(p, 8, p, p, p, 1, 1, 2, p, p, p, p, p, p, p, None) == -1
    assert L.spx_parse_mgf_text(p, 8, None, p, p, 1, 1, 0, p, p, p, p, p, p, p, None) == -1
    assert b"spx_parse_mgf_text" in L.spx_last_error()


# ------------------------------------------------------------------ random grammar
def _rand_num(rng, v, allow_exotic):
    forms = [lambda: f"{v:.5f}", lambda: repr(float(v)), lambda: f"{v:.2f}", lambda: str(int(v)),
             lambda: f"{v:.17g}", lambda: f"{v:.8f}".rstrip("0")]
    if allow_exotic:
        forms += [lambda: f"{v:.3e}", lambda: f"+{v:.4f}", lambda: f"{v:.4E}", lambda: f"{int(v)}."]
    return forms[int(rng.integers(0, len(forms)))]()


def _rand_mgf(rng, general):
    """Random MGF text in the shapes real files take (the generator shapes of
    tests/test_mgf_native.py): CRLF / CR / LF line ends, trailing blanks, extra peak
    fields, tab or double separators, exotic number forms, optional params, blank
    lines."""
    eol = ["\n", "\r\n", "\r"][int(rng.integers(0, 3))] if rng.random() < 0.3 else "\n"
    out = []
    for k in range(int(rng.integers(1, 6))):
        out.append("BEGIN IONS")
        out.append(f"TITLE=cluster-{k % 3};mzspec:X:{k}" + (" " if rng.random() < 0.1 else ""))
        if rng.random() < 0.9:
            out.append("PEPMASS=" + _rand_num(rng, rng.uniform(300, 1500), rng.random() < 0.3))
        if rng.random() < 0.9:
            out.append("CHARGE=" + ["2+", "3+", "2", " 2+ "][int(rng.integers(0, 4))])
        if rng.random() < 0.5:
            out.append("RTINSECONDS=" + _rand_num(rng, rng.uniform(0, 3600), False))
        for _ in range(int(rng.integers(0, 30))):
            a = _rand_num(rng, rng.uniform(100, 2000), rng.random() < 0.05)
            b = _rand_num(rng, rng.lognormal(3, 2), rng.random() < 0.05)
            r = rng.random()
            if general:
                sep = " " if r < 0.85 else ["\t", "  ", " \t"][int(rng.integers(0, 3))]
            else:
                sep = " " if r < 0.97 else ["\t", "  "][int(rng.integers(0, 2))]
            line = a + sep + b
            if rng.random() < 0.05:
                line += " 7"
            if rng.random() < 0.05:
                line += " "
            out.append(line)
            if rng.random() < 0.02:
                out.append("")
        out.append("END IONS")
        out.append("")
    return eol.join(out) + eol


@pytest.mark.parametrize("general", [False, True])
def test_random_mgf_text_device_equals_host(gpu, tmp_path, general):
    rng = np.random.default_rng(21 + general)
    n_equal = n_ok = 0
    for i in range(60):
        p = tmp_path / f"r{i}.mgf"
        p.write_bytes(_rand_mgf(rng, general).encode())
        X = mgf_native.index(str(p), general)
        order = rng.permutation(len(X["begin"]))
        status = _both(p, X, order, general, gpu, f"file {i}", fallback_ok=True)
        n_equal += _host(p, X["begin"], X["end"], general) is not None
        n_ok += int((status == OK).sum())
    assert n_equal > 15 and n_ok > 30  # both outcomes occur, and the kernel decides records itself


# ------------------------------------------------------------------ CLIs
@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    return synthetic_mgf(str(tmp_path_factory.mktemp("syn") / "clustered.mgf"), n_clusters=60, seed=5)


@pytest.fixture
def loads(monkeypatch):
    """SPX_DEVICE_INGEST=1, and what every device_ingest.load returned."""
    seen = []
    real = device_ingest.load

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append(r)
        return r

    monkeypatch.setenv(device_ingest.ENV, "1")
    monkeypatch.setattr(device_ingest, "load", spy)
    return seen


def _quiet(fn, *a, **k):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        fn(*a, **k)
    return out.getvalue()


@pytest.mark.parametrize("name", ["bin_mean_cli", "bin_mean_cli_nonfinite"])
def test_binning_cli_byte_identical(gpu, tmp_path, loads, name):
    out = tmp_path / "out.mgf"
    _quiet(binning.main, ["--mgf_file", os.path.join(GOLDEN, name + "_in.mgf"), "--out", str(out)])
    assert out.read_bytes() == open(os.path.join(GOLDEN, name + "_out.mgf"), "rb").read()
    assert len(loads) == 1
    if name == "bin_mean_cli":
        assert loads[0] is not None and loads[0][1]["n_reparse"] == 0
    else:  # nan / inf tokens: outside the host parser's subset as well, today's path decides
        assert loads[0] is None


def test_binning_cli_noncontiguous_clusters(gpu, tmp_path, syn, loads, monkeypatch):
    on, off = tmp_path / "on.mgf", tmp_path / "off.mgf"
    _quiet(binning._main_mgf, syn, str(on), 1)
    assert loads[0] is not None
    monkeypatch.delenv(device_ingest.ENV)
    _quiet(binning._main_mgf, syn, str(off), 1)
    assert len(loads) == 1 and on.read_bytes() == off.read_bytes()


@pytest.mark.parametrize("modes", [("lower_median", "mass_lower_median"), ("naive_average", "median"),
                                   ("neutral_average", "median"), ("naive_average", "mass_lower_median")])
@pytest.mark.parametrize("which", ["golden", "syn"])
def test_gap_average_cli_identical_to_host_ingest(gpu, tmp_path, syn, loads, monkeypatch, which, modes):
    src = syn if which == "syn" else os.path.join(GOLDEN, "bin_mean_cli_in.mgf")
    on, off = tmp_path / "on.mgf", tmp_path / "off.mgf"
    args = ["--encodedclusters", "--pepmass", modes[0], "--rt", modes[1]]
    asc.main([src, str(on)] + args)
    assert loads[0] is not None
    monkeypatch.delenv(device_ingest.ENV)
    asc.main([src, str(off)] + args)
    assert len(loads) == 1 and on.read_bytes() == off.read_bytes() and len(on.read_bytes()) > 0


@pytest.mark.parametrize("which", ["golden", "syn"])
def test_medoid_cli_identical_to_host_ingest(gpu, tmp_path, syn, loads, monkeypatch, which):
    src = syn if which == "syn" else os.path.join(GOLDEN, "medoid_noncontiguous.mgf")
    on, off = tmp_path / "on.mgf", tmp_path / "off.mgf"
    said_on = _quiet(msr.main, ["-i", src, "-o", str(on)])
    assert loads[0] is not None
    monkeypatch.delenv(device_ingest.ENV)
    said_off = _quiet(msr.main, ["-i", src, "-o", str(off)])
    assert len(loads) == 1 and said_on == said_off
    assert on.read_bytes() == off.read_bytes() and len(on.read_bytes()) > 0


def test_clis_outside_the_subset_take_todays_path(gpu, tmp_path, loads, monkeypatch):
    """Several charges (the dict path decides), a binning title without ';' (the
    reference's IndexError): the same result or exception as without the switch."""
    text = open(os.path.join(GOLDEN, "medoid_noncontiguous.mgf")).read()
    several = tmp_path / "several.mgf"
    several.write_text(text.replace("CHARGE=2+", "CHARGE=2+ and 3+", 1))
    notitle = tmp_path / "notitle.mgf"
    notitle.write_text(open(os.path.join(GOLDEN, "bin_mean_cli_in.mgf")).read().replace(";", ":", 1))
    on, off = tmp_path / "on.mgf", tmp_path / "off.mgf"
    said_on = _quiet(msr.main, ["-i", str(several), "-o", str(on)])
    with pytest.raises(IndexError):
        _quiet(binning._main_mgf, str(notitle), str(tmp_path / "x.mgf"), 1)
    assert loads == [None, None]
    monkeypatch.delenv(device_ingest.ENV)
    said_off = _quiet(msr.main, ["-i", str(several), "-o", str(off)])
    assert said_on == said_off and on.read_bytes() == off.read_bytes()
    with pytest.raises(IndexError):
        _quiet(binning._main_mgf, str(notitle), str(tmp_path / "y.mgf"), 1)
