"""The fused pass's step bodies after their instruction diet (bin_mean.hip phases A-C,
fused.hip medoid_from_codes), on the inputs of tests/fused_diet_cases.py (whose properties
tests/test_fused_diet_inputs.py proves on the host).

The diet changed how a lane without a contribution behaves (it issues no LDS atomic where
it ORed 0 into a word of its own), where a NaN is noticed (on the division path), how a
code is packed (one v_alignbit in phase A, one v_perm in phase C), how a step learns its
spectrum's length (one carried v_readlane) and where the rows' offset lives (a scalar
register, reloaded per cluster).  Each batch goes through test_gpu_fused._check: the C
oracle, the two separate entry points, unchecked and reused outputs, all bit for bit.
"""
import numpy as np
import pytest

import fused_diet_cases as dc
from test_gpu_fused import _check, _clean_flags
from test_gpu_fused_persistent import fu_grid

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", [dc.NO_QUORUM, {}], ids=["noquorum", "quorum"])
def test_band_edges_decide_bins(gpu, kw):
    """m/z whose reciprocal-product fraction is 0, inside either band, the last inside and
    the first outside, for both bin functions: the division path and the fast path next to
    it each decide bins, and a peak binned on the wrong side changes a mean or a distance."""
    csr, f = dc.case("band_edges")
    batch, got, rep, tot = _check(csr, kw, dc.TOL)
    assert _clean_flags(batch) == [True]  # decided in the register bodies, not handed on


def test_lanes_and_waves_with_nothing_to_or(gpu):
    """Spectra of 1, 62, 63, 64, 126, 127, 189, 190 and 252 peaks, one whose 40 peaks share
    one bin of each kind, and a cluster wholly out of range (no lane ever contributes)."""
    csr, f = dc.case("idle_lanes")
    batch, got, rep, tot = _check(csr, {}, dc.TOL)
    c = f["all_out"]
    assert got["out_off"][c + 1] == got["out_off"][c] and got["status"][c] == 0
    assert _clean_flags(batch) == [True]


def test_last_in_bin_across_wave_seams(gpu):
    """Peaks 62|63, 125|126 and 188|189 in one bin (lane 62 is not the last of its bin)
    and in two."""
    csr, f = dc.case("seams")
    batch, *_ = _check(csr, dc.NO_QUORUM, dc.TOL)
    assert _clean_flags(batch) == [True]


def test_code_packing_at_its_largest_values(gpu):
    """n = 1, 2, 3, 49, 50 with slots up to 1,529 and columns up to 1,719 (n >= 49) or all
    that n spectra hold: both halves of a code full, the last odd spectrum unpaired."""
    csr, f = dc.case("packing")
    batch, got, rep, tot = _check(csr, dc.NO_QUORUM, dc.TOL)
    for c, n in f["sizes"].items():
        want = 1530 if n >= 49 else 252 * n
        assert got["out_off"][c + 1] - got["out_off"][c] == want
    assert _clean_flags(batch) == [True]


@pytest.mark.parametrize("grid", [1, 2])
def test_one_sequence_under_a_small_grid(gpu, grid):
    """All of the above with a kNotHere and a mixed-charge cluster between them, walked by
    one and by two workgroups: what a step body holds per cluster (the rows' scalar
    offset, the carried spectrum start) is set again after every kind of early exit."""
    csr, f = dc.case("sequence")
    with fu_grid(grid):
        batch, got, rep, tot = _check(csr, {}, dc.TOL)
    assert np.all(rep >= 0)
