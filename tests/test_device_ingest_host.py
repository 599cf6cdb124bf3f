"""The host side of the opt-in device ingest (specpride_amd/device_ingest.py): the
destination order it hands the kernel, the argument checks of the C-ABI entry
point that need no device, the switch and the preamble check.  The kernel itself
is tested on the GPU (tests/test_gpu_device_ingest.py)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from specpride_amd import _lib, device_ingest, ingest, mgf_native
from test_sharded_cli import synthetic_mgf

MODES = [(mgf_native.GROUP_BINNING, False, ingest.binning_groups),
         (mgf_native.GROUP_RUNS, True, ingest.gap_average_groups),
         (mgf_native.GROUP_FIRST_RUNS, True, ingest.medoid_groups)]


@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    return synthetic_mgf(str(tmp_path_factory.mktemp("syn") / "clustered.mgf"), n_clusters=40, seed=4)


@pytest.mark.parametrize("mode,general,groups", MODES, ids=["binning", "runs", "first_runs"])
@pytest.mark.parametrize("which", ["syn", "medoid_noncontiguous.mgf", "bin_mean_cli_in.mgf"])
def test_plan_equals_csr_from_flat(syn, which, mode, general, groups):
    """The record permutation and the destination-order spec_off the kernel gets are
    the ones ingest.csr_from_flat builds from a host parse of the same file."""
    path = syn if which == "syn" else os.path.join(GOLDEN, which)
    X = mgf_native.index(path, general)
    flat = mgf_native.parse_ranges(path, X["begin"], X["end"], general)  # file order
    ids, records, sizes = groups(X["titles"])
    want = ingest.csr_from_flat(flat, sizes, records)
    got_ids, got_sizes, order, n_used, spec_off = device_ingest.plan(X["titles"], X["npk"], mode)
    assert got_ids == ids and n_used == len(records)
    np.testing.assert_array_equal(got_sizes, sizes)
    np.testing.assert_array_equal(order[:n_used], records)
    np.testing.assert_array_equal(np.sort(order), np.arange(len(X["titles"])))  # every record is parsed once
    np.testing.assert_array_equal(spec_off[:n_used + 1], want.spec_off)
    np.testing.assert_array_equal(ingest.cluster_starts(got_sizes), want.cluster_off)
    np.testing.assert_array_equal(np.diff(spec_off), X["npk"][order])
    if mode == mgf_native.GROUP_FIRST_RUNS and which != "bin_mean_cli_in.mgf":
        assert n_used < len(order)  # later runs: parsed (the host parses them too), outside the CSR


def test_entry_point_rejects_bad_sizes_without_a_device():
    """Negative sizes, a grammar other than 0/1 and null arrays are SPX_EINVAL before
    any HIP call (the byte ranges themselves live in device memory: the kernel
    flags those per record)."""
    L = ctypes.CDLL(_lib.build())
    L.spx_last_error.restype = ctypes.c_char_p
    p, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    f = L.spx_parse_mgf_text
    f.argtypes = [p, i64, p, p, p, i64, i64, i32, p, p, p, p, p, p, p, p]
    buf = (ctypes.c_int64 * 8)()
    a = ctypes.addressof(buf)  # never dereferenced: every call below fails its checks
    EINVAL = -1
    assert f(a, -1, a, a, a, 1, 1, 0, a, a, a, a, a, a, a, None) == EINVAL
    assert f(a, 8, a, a, a, -1, 1, 0, a, a, a, a, a, a, a, None) == EINVAL
    assert f(a, 8, a, a, a, 1, -1, 0, a, a, a, a, a, a, a, None) == EINVAL
    assert f(a, 8, a, a, a, 1, 1, 2, a, a, a, a, a, a, a, None) == EINVAL
    assert f(None, 8, a, a, a, 1, 1, 0, a, a, a, a, a, a, a, None) == EINVAL
    assert f(a, 8, a, a, a, 1, 1, 0, None, a, a, a, a, a, a, None) == EINVAL
    for k in (2, 3, 4, 10, 11, 12, 13, 14):
        args = [a, 8, a, a, a, 1, 1, 0, a, a, a, a, a, a, a, None]
        args[k] = None
        assert f(*args) == EINVAL, k
        assert b"spx_parse_mgf_text" in L.spx_last_error()
    assert f(None, 0, None, None, None, 0, 0, 1, None, None, None, None, None, None, None, None) == 0  # nothing to do


def test_switch_is_opt_in(monkeypatch):
    monkeypatch.delenv(device_ingest.ENV, raising=False)
    assert not device_ingest.enabled()
    monkeypatch.setenv(device_ingest.ENV, "0")
    assert not device_ingest.enabled()
    monkeypatch.setenv(device_ingest.ENV, "1")
    assert device_ingest.enabled()


@pytest.mark.parametrize("pre,general,ok", [
    ("", False, True), ("\n\r\n", False, True), ("BEGIN IONS\n", False, True), ("BEGIN IONS\r\n\r\n", False, True),
    ("PEPMASS=5\n", False, False), ("12 3\n", False, False), ("END IONS\n", False, False), ("# x\n", False, False),
    ("COM=demo\nMASS=Monoisotopic\n", True, True), ("END IONS\n", True, False), ("café\n", True, False),
])
def test_preamble_check(tmp_path, pre, general, ok):
    """Bytes before the first indexed record: only what the whole-file host parsers
    pass over lets the device path run."""
    path = tmp_path / "p.mgf"
    data = pre.encode("utf-8")
    path.write_bytes(data + b"TITLE=a;b\nEND IONS\n")
    assert device_ingest._preamble_ok(str(path), len(data), general) is ok
