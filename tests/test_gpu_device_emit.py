"""Device-side MGF emit (specpride_amd/device_emit.py, csrc/mgf_format.hip) against
its oracles: ``spx_format_peaks`` against Python's own ``repr`` per segment (text and
offsets exactly), and the binning and gap-average CLIs with ``SPX_DEVICE_EMIT=1``
against the same CLI with the switch off (``mgf_native.write_records``), byte for
byte, with and without ``SPX_DEVICE_INGEST=1``.
"""
import contextlib
import io
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from specpride_amd import average_spectrum_clustering as asc
from specpride_amd import binning, device_emit, device_ingest, engine
from test_sharded_cli import synthetic_mgf

pytestmark = pytest.mark.gpu

P = 100_000  # peaks of the shared pool: 2 * 10^5 values
NAN_MZ = 5000  # the peak "nan 5.0"
CAPACITY, RANGE = engine.FORMAT_FLAG_CAPACITY, engine.FORMAT_FLAG_RANGE


def _pool():
    """P peaks whose neighbours differ in class -- the value classes of
    tests/test_repr_core.py -- so neighbouring lanes' values take 3 to 24 bytes and
    their lines 8 ("5.0 0.0") to 50 ("-2.2250738585072014e-308 -1.7976931348623157e+308")."""
    rng = np.random.default_rng(77)
    n = 2 * P
    k = rng.integers(1, 51, n)
    classes = [
        rng.uniform(50, 3000, n),
        (rng.uniform(50, 3000, n) * k).astype(np.float32).astype(np.float64) / k,
        rng.lognormal(3, 3, n),
        10.0 ** rng.uniform(-320, 308, n) * rng.choice([-1.0, 1.0], n),
        rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64),
        rng.integers(0, 10, n).astype(np.float64),  # "5.0": the shortest lines
        np.round(rng.uniform(0, 2000, n), 2),
    ]
    listed = [math.ldexp(1.0, e) for e in range(-1074, 1024, 7)]
    listed += [math.nextafter(v, math.inf) for v in listed[::3]] + [math.nextafter(v, 0.0) for v in listed[::3]]
    listed += [1e-5, 9.999e-5, 1e-4, 0.001, 1e15, 9999999999999998.0, 1e16, 1e17, 1e21, 1e22, 1e23, 5e-324,
               2.2250738585072014e-308, 1.7976931348623157e308, 0.0, -0.0, 0.1, 0.3, 2 / 3, 123456789012345680.0,
               math.nan, math.inf, -math.inf, -2.2250738585072014e-308, -1.7976931348623157e308]
    which = rng.integers(0, len(classes), n)
    vals = np.choose(which, classes)
    at = rng.choice(n, len(listed), replace=False)
    vals[at] = listed
    vals[:2] = [-2.2250738585072014e-308, -1.7976931348623157e308]  # one 50-byte line
    vals[2:4] = [1.0, 2.0]
    mz, inten = vals[0::2].copy(), vals[1::2].copy()
    mz[NAN_MZ], inten[NAN_MZ] = math.nan, 5.0  # a NaN m/z is printed whatever skip_nan says
    return mz, inten


class Pool:
    """The pool on the host and the device, and its reference lines (made once)."""

    def __init__(self, gpu):
        import torch

        self.mz, self.inten = _pool()
        self.lines = [f"{m!r} {i!r}\n".encode() for m, i in zip(self.mz.tolist(), self.inten.tolist())]
        self.dmz = torch.from_numpy(self.mz).to(gpu)
        self.dint = torch.from_numpy(self.inten).to(gpu)
        self.gpu = gpu

    def want(self, begin, end, inten=None, skip_nan=False):
        """(text, text_off) of the segments from Python's repr; a bad range is empty."""
        it = self.inten if inten is None else inten
        blocks = []
        for b, e in zip(begin, end):
            if b < 0 or e < b or e > len(self.mz):
                blocks.append(b"")
            elif inten is None and not skip_nan:
                blocks.append(b"".join(self.lines[b:e]))
            else:
                blocks.append(b"".join(f"{float(self.mz[k])!r} {float(it[k])!r}\n".encode() for k in range(b, e)
                                       if not (skip_nan and math.isnan(it[k]))))
        off = np.zeros(len(blocks) + 1, np.int64)
        np.cumsum([len(b) for b in blocks], out=off[1:])
        return b"".join(blocks), off

    def run(self, begin, end, dint=None, **kw):
        import torch

        sb = torch.tensor(list(begin), dtype=torch.int64, device=self.gpu)
        se = torch.tensor(list(end), dtype=torch.int64, device=self.gpu)
        return engine.format_peaks(self.dmz, self.dint if dint is None else dint, sb, se, **kw)


@pytest.fixture(scope="module")
def pool(gpu):
    return Pool(gpu)


def _check(pool, begin, end, flags=0, inten=None, dint=None, **kw):
    h = pool.run(begin, end, dint=dint, **kw).to_host()
    text, off = pool.want(begin, end, inten=inten, skip_nan=kw.get("skip_nan", False))
    assert h["flags"] == flags
    np.testing.assert_array_equal(h["text_off"], off)
    assert h["text"].tobytes() == text
    return h


def _consecutive(lengths, start=0):
    begin = start + np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return begin.tolist(), (begin + np.asarray(lengths)).tolist()


EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def test_pool_lines_span_8_to_50_bytes(pool):
    n = np.array([len(ln) for ln in pool.lines])
    assert n.max() == 50 and n.min() == 8
    assert np.abs(np.diff(n)).mean() > 4  # neighbours differ


def test_segment_lengths_around_wave_block_and_tile(pool):
    b, e = _consecutive(EDGE_LENGTHS)
    _check(pool, b, e)
    _check(pool, b[::-1], e[::-1])  # out of order
    for n in EDGE_LENGTHS:  # and each alone, from an odd start
        _check(pool, [7], [7 + n])


def test_giant_segment_between_one_peak_segments(pool):
    b, e = _consecutive([1, 1, 70000, 1, 1], start=5000)
    h = _check(pool, b, e)
    assert h["text_off"][3] - h["text_off"][2] > 70000 * 20


def test_overlapping_out_of_order_and_empty_runs(pool):
    begin = [10, 100, 0, 90000, 300]
    end = [500, 700, 1025, 90001, 300]
    begin += [4242] * 3000  # 3,000 empty segments in a row
    end += [4242] * 3000
    begin += [50, 0, 99999, 100000]
    end += [60, 0, 100000, 100000]  # ... then text again, and empty segments at the very end
    _check(pool, begin, end)
    _check(pool, [P] * 5, [P] * 5)  # nothing but empty segments


def test_thousands_of_small_segments(pool):
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 4, 20000)
    b, e = _consecutive(lengths, start=123)
    perm = rng.permutation(len(b))
    _check(pool, np.asarray(b)[perm].tolist(), np.asarray(e)[perm].tolist())


def test_nan_intensities_skipped_or_printed(pool):
    import torch

    inten = pool.inten.copy()
    begin = [0, 100, 300, 364, 1000, 1100, 1101, 1300]
    end = [100, 300, 364, 700, 1100, 1101, 1300, 1301]
    inten[0] = inten[99] = np.nan           # first and last peak of a segment
    inten[100:300] = np.nan                 # a whole segment
    inten[301:700:2] = np.nan               # every other peak, across wave and tile boundaries
    inten[1100] = np.nan                    # a one-peak segment that vanishes
    inten[1300] = np.nan
    begin.append(NAN_MZ)                    # a NaN m/z is printed either way
    end.append(NAN_MZ + 1)
    dint = torch.from_numpy(inten).to(pool.gpu)
    skipped = _check(pool, begin, end, inten=inten, dint=dint, skip_nan=True)
    printed = _check(pool, begin, end, inten=inten, dint=dint, skip_nan=False)
    assert skipped["text_off"][2] == skipped["text_off"][1] and skipped["text_off"][6] == skipped["text_off"][5]
    n_nan = sum(int(np.isnan(inten[b:e]).sum()) for b, e in zip(begin, end))
    assert n_nan >= 2 + 200 + 200 + 2 and printed["text"].tobytes().count(b" nan\n") == n_nan
    assert skipped["text"].tobytes().count(b" nan\n") == 0
    for h in (skipped, printed):
        assert h["text"].tobytes()[h["text_off"][-2]:] == b"nan 5.0\n"


def test_capacity_exact_and_one_byte_short(pool):
    import torch

    b, e = _consecutive([3, 0, 700, 65], start=40)
    text, off = pool.want(b, e)
    need = len(text)
    guard = 256
    buf = torch.full((need + guard,), 0xAB, dtype=torch.uint8, device=pool.gpu)
    out = engine.FormatResult(buf, torch.empty(len(b) + 1, dtype=torch.int64, device=pool.gpu),
                              torch.ones(1, dtype=torch.int32, device=pool.gpu))
    h = pool.run(b, e, out=out, capacity=need).to_host()
    assert h["flags"] == 0 and h["text"].tobytes() == text
    assert (buf[need:] == 0xAB).all().item()
    buf.fill_(0xAB)
    h = pool.run(b, e, out=out, capacity=need - 1).to_host()
    assert h["flags"] == CAPACITY and len(h["text"]) == 0
    np.testing.assert_array_equal(h["text_off"], off)  # still says what is needed
    assert (buf[need - 1:] == 0xAB).all().item()       # nothing at or past the capacity
    # the default capacity (50 bytes per covered peak) always suffices
    assert pool.run(b, e).to_host()["flags"] == 0


def test_bad_ranges_are_flagged_and_empty(pool):
    begin = [0, -1, 50, 20, P - 5, 60, P + 1]
    end = [10, 5, 40, 30, P + 1, 70, P + 2]
    h = _check(pool, begin, end, flags=RANGE)
    off = h["text_off"]
    assert off[2] == off[1] and off[3] == off[2] and off[5] == off[4] and off[7] == off[6]
    _check(pool, [0, 20], [10, 30], flags=0)


def test_empty_inputs_and_host_checked_arguments(pool, gpu):
    import torch

    from specpride_amd import _lib

    none = torch.empty(0, dtype=torch.int64, device=gpu)
    h = engine.format_peaks(pool.dmz, pool.dint, none, none).to_host()
    assert h["flags"] == 0 and h["text_off"].tolist() == [0] and len(h["text"]) == 0
    nopeaks = torch.empty(0, dtype=torch.float64, device=gpu)
    z = torch.zeros(3, dtype=torch.int64, device=gpu)
    h = engine.format_peaks(nopeaks, nopeaks, z, z).to_host()
    assert h["flags"] == 0 and h["text_off"].tolist() == [0, 0, 0, 0]
    h = engine.format_peaks(nopeaks, nopeaks, z, z + 1).to_host()  # every range is past n_peaks = 0
    assert h["flags"] == RANGE and h["text_off"].tolist() == [0, 0, 0, 0]
    L = _lib.lib()
    t = torch.zeros(4096, dtype=torch.int64, device=gpu)
    p = t.data_ptr()
    need = L.spx_format_peaks_workspace_size(4, 16)
    assert 0 < need <= t.numel() * 8
    ok = (p, p, 16, p, p, 4, 0, p, 64, p, p, p, need, None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.spx_format_peaks(*a)

    assert call(a0=None) == -1 and call(a3=None) == -1 and call(a9=None) == -1 and call(a10=None) == -1
    assert call(a2=-1) == -1 and call(a5=-1) == -1 and call(a8=-1) == -1 and call(a7=None) == -1
    assert call(a12=need - 1) == -1 and call(a11=None) == -1
    assert b"spx_format_peaks" in L.spx_last_error()
    assert L.spx_format_peaks_workspace_size(-1, 0) == 0


def test_captured_on_a_side_stream_and_replayed(pool):
    import torch

    b, e = _consecutive([5, 300, 0, 1025, 64], start=900)
    text, off = pool.want(b, e)
    sb = torch.tensor(b, dtype=torch.int64, device=pool.gpu)
    se = torch.tensor(e, dtype=torch.int64, device=pool.gpu)
    side = torch.cuda.Stream(device=pool.gpu)
    side.wait_stream(torch.cuda.current_stream(pool.gpu))
    with torch.cuda.stream(side):
        out = engine.format_peaks(pool.dmz, pool.dint, sb, se, capacity=len(text) + 64)  # sizes every buffer
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            engine.format_peaks(pool.dmz, pool.dint, sb, se, out=out)
        for _ in range(2):
            out.text.zero_()
            out.text_off.zero_()
            graph.replay()
            side.synchronize()
            h = out.to_host()
            assert h["flags"] == 0 and h["text"].tobytes() == text
            np.testing.assert_array_equal(h["text_off"], off)
    torch.cuda.current_stream(pool.gpu).wait_stream(side)


# ------------------------------------------------------------------ CLIs
@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    return synthetic_mgf(str(tmp_path_factory.mktemp("syn_emit") / "clustered.mgf"), n_clusters=300, seed=9)


@pytest.fixture
def emits(monkeypatch):
    """What every device_emit.write_records call wrote to (the switch itself is set per arm)."""
    seen = []
    real = device_emit.write_records

    def spy(path, *a, **k):
        seen.append(path)
        return real(path, *a, **k)

    monkeypatch.setattr(device_emit, "write_records", spy)
    return seen


def _arm(monkeypatch, run, out, emit):
    """One CLI run: (stdout, output bytes or None, exception or None)."""
    if emit:
        monkeypatch.setenv(device_emit.ENV, "1")
    else:
        monkeypatch.delenv(device_emit.ENV, raising=False)
    said, err = io.StringIO(), None
    with contextlib.redirect_stdout(said):
        try:
            run(str(out))
        except Exception as e:  # noqa: BLE001 -- compared between the arms
            err = (type(e), str(e))
    return said.getvalue(), (out.read_bytes() if out.exists() else None), err


def _both_arms(monkeypatch, tmp_path, run, ingest):
    if ingest:
        monkeypatch.setenv(device_ingest.ENV, "1")
    else:
        monkeypatch.delenv(device_ingest.ENV, raising=False)
    on = _arm(monkeypatch, run, tmp_path / "on.mgf", True)
    off = _arm(monkeypatch, run, tmp_path / "off.mgf", False)
    assert on[2] == off[2], "the two arms raise differently"
    assert on[0] == off[0]
    if on[2] is not None:
        assert on[1] is None, "an error was raised after the output was written"
    else:
        assert on[1] == off[1]
    return on


INPUTS = ["bin_mean_cli_in.mgf", "bin_mean_cli_nonfinite_in.mgf", "medoid_noncontiguous.mgf", "best_spectrum_in.mgf",
          "SYN"]
EMITTED = ["bin_mean_cli_in.mgf", "SYN"]  # inside the native subset of every CLI: the device must have written them


def _src(name, syn):
    return syn if name == "SYN" else os.path.join(GOLDEN, name)


@pytest.mark.parametrize("ingest", [False, True], ids=["host_ingest", "device_ingest"])
@pytest.mark.parametrize("name", INPUTS)
def test_binning_cli_byte_identical(gpu, tmp_path, monkeypatch, emits, syn, name, ingest):
    src = _src(name, syn)
    said, data, err = _both_arms(monkeypatch, tmp_path, lambda out: binning.main(["--mgf_file", src, "--out", out]),
                                 ingest)
    if name.startswith("bin_mean_cli"):
        assert err is None
        assert data == open(os.path.join(GOLDEN, name.replace("_in.mgf", "_out.mgf")), "rb").read()
    if name in EMITTED:
        assert emits == [str(tmp_path / "on.mgf")]


@pytest.mark.parametrize("ingest", [False, True], ids=["host_ingest", "device_ingest"])
@pytest.mark.parametrize("name", INPUTS)
def test_gap_average_cli_byte_identical(gpu, tmp_path, monkeypatch, emits, syn, name, ingest):
    src = _src(name, syn)
    _said, data, err = _both_arms(monkeypatch, tmp_path, lambda out: asc.main([src, out, "--encodedclusters"]), ingest)
    if name in EMITTED:
        assert err is None and len(data) > 0 and emits == [str(tmp_path / "on.mgf")]


@pytest.mark.parametrize("ingest", [False, True], ids=["host_ingest", "device_ingest"])
def test_gap_average_cli_appends(gpu, tmp_path, monkeypatch, emits, syn, ingest):
    head = b"BEGIN IONS\nTITLE=kept\n1.0 2.0\nEND IONS\n\n"

    def run(out):
        with open(out, "wb") as fh:
            fh.write(head)
        asc.main([syn, out, "--encodedclusters", "--append", "--pepmass", "naive_average", "--rt", "median"])

    _said, data, err = _both_arms(monkeypatch, tmp_path, run, ingest)
    assert err is None and data.startswith(head) and len(data) > len(head) and len(emits) == 1


@pytest.mark.parametrize("ingest", [False, True], ids=["host_ingest", "device_ingest"])
def test_mixed_charge_raises_before_anything_is_written(gpu, tmp_path, monkeypatch, emits, ingest):
    text = open(os.path.join(GOLDEN, "bin_mean_cli_in.mgf")).read()
    at = text.index("CHARGE=")
    eol = text.index("\n", at)
    old = text[at:eol]
    mixed = tmp_path / "mixed.mgf"
    mixed.write_text(text[:at] + ("CHARGE=7+" if old != "CHARGE=7+" else "CHARGE=6+") + text[eol:])
    _said, data, err = _both_arms(monkeypatch, tmp_path,
                                  lambda out: binning.main(["--mgf_file", str(mixed), "--out", out]), ingest)
    assert err == (AssertionError, binning.MIXED_CHARGE_MSG) and data is None and emits == []
