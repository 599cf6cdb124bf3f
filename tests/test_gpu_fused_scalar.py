"""The fused pass after its set-up and scalar-stream changes (bin_mean.hip
bin_mean_reg_path_t, fused.hip), on the inputs of tests/fused_scalar_cases.py (whose
properties tests/test_fused_scalar_inputs.py proves on the host).

Phase A's first ring loads now go out ahead of the set-up's LDS work, so every return
between the header checks and the first step is taken with loads in flight, and the two
reciprocal products' band edges sit in scalar registers for the whole cluster.  Each batch
goes through test_gpu_fused._check: the C oracle and the two separate entry points
(engine.bin_mean + engine.medoid), counts, f64 peak bits, rep, status, prec and charge,
checked and unchecked, on fresh and on reused outputs, all bit for bit.
"""
import numpy as np
import pytest

import fused_scalar_cases as sc
from specpride_amd import engine
from test_gpu_fused import _assert_bm_bits, _assert_md_bits, _check, _clean_flags, _md_host
from test_gpu_fused_persistent import fu_grid

pytestmark = pytest.mark.gpu


def test_lane_mask_edges_and_empty_spectra(gpu):
    """Spectra of 1, 62, 63, 64, 125, 126, 127, 188, 189, 190, 251 and 252 peaks, each
    length alone in a cluster and all in one (a wave's owned lanes empty, full, or one lane),
    and a zero-length spectrum first, in the middle and last in a cluster."""
    csr, f = sc.case("mask_edges")
    batch, got, rep, tot = _check(csr, {}, sc.TOL)
    assert np.all(got["status"] == 0) and np.all(rep >= 0)
    assert _clean_flags(batch) == [True]  # every cluster completed in the register bodies


def test_ring_depth_edges(gpu):
    """n = 1, 2, 5, 6, 7, 12, 13 around the ring's depth of 6; n = 50 completes the register
    path, n = 51 is handed on; a 253-peak spectrum (kNotHere) with a normal cluster after it."""
    csr, f = sc.case("ring_depths")
    batch, got, rep, tot = _check(csr, {}, sc.TOL)
    assert np.all(got["status"] == 0) and np.all(rep >= 0)


@pytest.mark.parametrize("kind", sc.EARLY_KINDS)
def test_early_returns_with_loads_in_flight(gpu, kind):
    """A mixed-charge cluster, an unsorted and a NaN m/z (kDeferred), more than 1,536 bins,
    a medoid bin outside [0, 32,768) and n = 1, each first, in the middle and last in its
    batch, on the default grid and walked by one workgroup."""
    csr, f = sc.case("early_returns", kind)
    want = None
    for grid in (None, 1):
        with fu_grid(grid):
            batch, got, rep, tot = _check(csr, {}, sc.TOL)
        if want is not None:
            _assert_bm_bits(got, want[0], f"grid {grid}")
            _assert_md_bits((rep, tot), want[1], f"grid {grid}")
        want = (got, (rep, tot))
    assert np.all(rep >= 0)


@pytest.mark.parametrize("name", ["walk", "walk_ends_off_path"])
def test_persistent_walk(gpu, name):
    """One workgroup walks the whole batch (SPX_FU_GRID=1), and two do: the same bits as
    the uncapped grid.  `walk_ends_off_path` ends in a cluster that leaves the stepped path."""
    csr, f = sc.case(name)
    batch, want, want_rep, want_tot = _check(csr, {}, sc.TOL)
    for grid in (1, 2):
        with fu_grid(grid):
            batch, got, rep, tot = _check(csr, {}, sc.TOL)
        _assert_bm_bits(got, want, f"grid {grid}")
        _assert_md_bits((rep, tot), (want_rep, want_tot), f"grid {grid}")


@pytest.mark.parametrize("C", [0, 1, 2])
def test_persistent_few_clusters(gpu, C):
    """0, 1 and 2 clusters under grids of 1 and 2 and the uncapped grid."""
    csr, _ = sc.case("few", C)
    results = []
    for grid in (None, 1, 2):
        with fu_grid(grid):
            if C == 0:  # nothing to launch: the call returns empty outputs
                bm, md = engine.bin_mean_medoid(engine.DeviceBatch.from_host(csr), tolerance=sc.TOL, with_totals=True)
                got = bm.to_host()
                assert got["out_off"][-1] == 0 and len(got["out_mz"]) == 0
                assert len(_md_host(md, csr)[0]) == 0
                continue
            batch, got, rep, tot = _check(csr, {}, sc.TOL)
        results.append((got, (rep, tot)))
    for got, md in results[1:]:
        _assert_bm_bits(got, results[0][0], "capped grid")
        _assert_md_bits(md, results[0][1], "capped grid")


def test_band_constants_follow_the_call(gpu):
    """One batch, in one process, under two BinMeanParams and two medoid tolerances in turn
    (A, B, A again, and the two crossed), with peaks exactly at, just below and just past the
    ends of both ranges and on bin edges of both grids that take the division: a band edge
    or parameter kept from another call or cluster would change a bin."""
    csr, f = sc.case("band_constants")
    runs = [(sc.PARAMS_A, sc.TOL_A), (sc.PARAMS_B, sc.TOL_B), (sc.PARAMS_A, sc.TOL_A),
            (sc.PARAMS_A, sc.TOL_B), (sc.PARAMS_B, sc.TOL_A)]
    seen = {}
    for q in (True, False):
        for kw, tol in runs:
            kw = dict(kw, apply_peak_quorum=q)
            batch, got, rep, tot = _check(csr, kw, tol)
            assert _clean_flags(batch) == [True]
            key = (kw["binsize"], tol, q)
            if key in seen:  # the same parameters again, after another set: the same bits
                _assert_bm_bits(got, seen[key][0], "repeated parameters")
                _assert_md_bits((rep, tot), seen[key][1], "repeated parameters")
            seen[key] = (got, (rep, tot))
    a, b = seen[(0.02, sc.TOL_A, True)], seen[(0.05, sc.TOL_B, True)]
    assert a[0]["out_off"][-1] != b[0]["out_off"][-1] and not np.array_equal(a[1][1], b[1][1])
