"""CPU tests of the host half of the device-side MGF emit: ``spx_repr_f64`` -- the
shortest-decimal core (csrc/repr_core.hpp) the format kernel runs, exported for the
host -- against Python's own ``repr``; the generated power-of-ten table against its
generator; and the splicing record writer (``spx_mgf_splice_records``) against
``mgf_native.write_records``, byte for byte.  No GPU is needed: both functions are
host code of libspecpride_hip.so."""
import ctypes
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from specpride_amd import _lib, device_emit, mgf_native


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _reprs(L, values):
    buf = ctypes.create_string_buffer(32)
    f = L.spx_repr_f64
    out = []
    for v in values:
        n = f(v, buf)
        assert 1 <= n <= 24, (v, n)
        out.append(buf.raw[:n])
    return out


def _mismatches(L, values):
    values = [float(v) for v in values]
    got = _reprs(L, values)
    return [(v.hex(), g, repr(v)) for v, g in zip(values, got) if g != repr(v).encode()]


def random_values(seed=2024):
    """The seeded set: > 10^6 doubles in the shapes the writers see, plus arbitrary ones."""
    rng = np.random.default_rng(seed)
    n = 220_000
    sums = rng.uniform(50, 3000, n) * rng.integers(1, 51, n)
    k = rng.integers(1, 51, n)
    decades = 10.0 ** rng.uniform(-320, 308, n)  # reaches into the subnormals
    bits = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    bits[:20000] &= np.uint64(0x800FFFFFFFFFFFFF)  # subnormals of both signs
    return np.concatenate([
        rng.uniform(50, 3000, n),
        sums.astype(np.float32).astype(np.float64) / k,  # f64(f32(sum)) / k: bin-mean outputs
        rng.lognormal(3, 3, n),
        decades * rng.choice([-1.0, 1.0], n),
        bits.view(np.float64),
    ])


def listed_values():
    vals = []
    for e in range(-1074, 1024):
        p = math.ldexp(1.0, e)
        vals += [p, math.nextafter(p, math.inf), math.nextafter(p, -math.inf)]
    vals += [1e-5, 9.999e-5, 1e-4, 0.001, 1e15, 9999999999999998.0, 1e16, 1e17, 1e21, 1e22, 1e23,
             5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 0.0, -0.0, 0.1, 0.3, 2 / 3,
             123456789012345680.0, math.nan, math.inf, -math.inf]
    vals += [float(i) for i in range(1, 10 ** 6, 997)]
    return vals + [-v for v in vals]


def test_repr_equals_python_on_a_million_seeded_doubles(L):
    vals = random_values()
    assert len(vals) >= 10 ** 6
    bad = _mismatches(L, vals.tolist())
    assert not bad, bad[:10]


def test_repr_equals_python_on_the_listed_values(L):
    bad = _mismatches(L, listed_values())
    assert not bad, bad[:10]
    assert _reprs(L, [1e-4, 123.45, 100.0, 9999999999999998.0, 1e16, 9.999e-05, 1e22, 5e-324, -0.0]) == \
        [b"0.0001", b"123.45", b"100.0", b"9999999999999998.0", b"1e+16", b"9.999e-05", b"1e+22", b"5e-324", b"-0.0"]
    assert max(len(r) for r in _reprs(L, [-2.2250738585072014e-308, -1.7976931348623157e308])) == 24


def test_generated_table_equals_the_committed_header():
    """The generator's output (Python integers) is the committed header, and its own
    enumeration of the core's fixed-point logarithms passes."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_repr_tables.py"), "--check"])
    assert r.returncode == 0


# ------------------------------------------------------------------ the splicing writer
def _records(rng, C, nan_every=0):
    """C records: titles with non-ASCII bytes, a 0-peak record, mixed value classes."""
    sizes = rng.integers(0, 40, C)
    sizes[min(2, C - 1)] = 0
    off = np.zeros(C + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    P = int(off[-1])
    mz = np.sort(rng.uniform(100, 2000, P))
    inten = rng.lognormal(3, 3, P)
    inten[::7] = np.round(inten[::7])
    inten[3::11] = 10.0 ** rng.uniform(-30, 30, len(inten[3::11]))
    if nan_every:
        inten[::nan_every] = np.nan
        if P:
            inten[off[1] - 1 if sizes[0] else 0] = np.nan
    titles = [f"cluster-{c};mzspec:PXDé中:{c}" if c % 3 else f"c{c}" for c in range(C)]
    titles[min(1, C - 1)] = "raw-\udcff\udc80-bytes"  # surrogate-escaped non-UTF-8 bytes
    prec = rng.uniform(300, 1500, C)
    prec[0] = 1e-7
    charge = rng.integers(-3, 5, C).astype(np.int64)
    rt = rng.uniform(0, 7200, C)
    rt[C - 1] = 1e22
    return titles, off, mz, inten, prec, charge, rt


def _host_text(L, off, mz, inten, skip_nan):
    """text_off / text of the peak lines, made on the host from spx_repr_f64."""
    C = len(off) - 1
    text_off = np.zeros(C + 1, np.int64)
    chunks = []
    for c in range(C):
        a, b = int(off[c]), int(off[c + 1])
        keep = [k for k in range(a, b) if not (skip_nan and math.isnan(inten[k]))]
        m, i = _reprs(L, [float(mz[k]) for k in keep]), _reprs(L, [float(inten[k]) for k in keep])
        block = b"".join(x + b" " + y + b"\n" for x, y in zip(m, i))
        chunks.append(block)
        text_off[c + 1] = text_off[c] + len(block)
    return text_off, np.frombuffer(b"".join(chunks), np.uint8)


@pytest.mark.parametrize("style", [0, 1, 2])
def test_splicing_writer_equals_native_writer(L, tmp_path, style):
    """Styles 0/1/2 with every flags combination, a 0-peak record, non-ASCII titles,
    NaN intensities (skipped by style 0, printed by 1 and 2), several writer blocks
    and thread counts, and append."""
    rng = np.random.default_rng(40 + style)
    C = 64
    titles, off, mz, inten, prec, charge, rt = _records(rng, C, nan_every=5)
    flags = np.array([c % 16 for c in range(C)], np.int32)  # all 16 combinations, four times
    text_off, text = _host_text(L, off, mz, inten, skip_nan=style == 0)
    for threads, use_flags in itertools.product((1, 3), (True, False)):
        f = flags if use_flags else None
        want, got = tmp_path / "want.mgf", tmp_path / "got.mgf"
        for append in (False, True):  # the second pass appends the same records again
            mgf_native.write_records(str(want), style, titles, off, mz, inten, prec, charge, rt, f, append=append,
                                     threads=threads)
            device_emit.splice_records(str(got), style, titles, text_off, text, prec, charge, rt, f, append=append,
                                       threads=threads)
            assert got.read_bytes() == want.read_bytes()
        assert want.read_bytes().count(b"BEGIN IONS") == 2 * C
        if style == 0:
            assert b"nan" not in got.read_bytes()
        else:
            assert b" nan\n" in got.read_bytes()


def test_splicing_writer_many_blocks(L, tmp_path):
    """More records than one writer round (2,048 per thread) holds."""
    rng = np.random.default_rng(50)
    C = 5000
    titles, off, mz, inten, prec, charge, rt = _records(rng, C)
    text_off, text = _host_text(L, off, mz, inten, skip_nan=False)
    want, got = tmp_path / "want.mgf", tmp_path / "got.mgf"
    mgf_native.write_records(str(want), 2, titles, off, mz, inten, prec, charge, rt, threads=2)
    device_emit.splice_records(str(got), 2, titles, text_off, text, prec, charge, rt, threads=2)
    assert got.read_bytes() == want.read_bytes()


def test_splicing_writer_rejects_bad_arguments_before_writing(L, tmp_path):
    path = tmp_path / "never.mgf"
    one = np.zeros(1)
    z = np.zeros(1, np.int64)
    with pytest.raises(ValueError):
        device_emit.splice_records(str(path), 0, ["a"], [0, 5], np.zeros(3, np.uint8), one, z)
    with pytest.raises(ValueError):
        device_emit.splice_records(str(path), 0, ["a\nb"], [0, 0], np.zeros(0, np.uint8), one, z)
    # decreasing offsets handed to the C entry point itself
    off = np.array([4, 2], np.int64)
    text = np.zeros(8, np.uint8)
    rc = L.spx_mgf_splice_records(os.fsencode(str(path)), 0, 0, 1, b"a", None, one.ctypes.data, z.ctypes.data, None,
                                  off.ctypes.data, text.ctypes.data, 1)
    assert rc == -1 and b"spx_mgf_splice_records" in L.spx_last_error()
    assert L.spx_mgf_splice_records(os.fsencode(str(path)), 0, 3, 0, b"", None, None, None, None, None, None, 1) == -1
    assert not path.exists()
