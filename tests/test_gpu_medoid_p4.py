"""The register tail past 32 spectra -- one Gram tile per wave, the hand-off between the two
waves of a column tile -- and the diagonal tiles' shared operand fragment (medoid_tail_regs,
csrc/medoid.hip) on the GPU: every case of tests/medoid_p4_cases.py through the fused pass
(test_gpu_fused._check: the C oracle, the separate entry points, checked and unchecked, fresh
and reused outputs, totals included) and through engine.medoid alone, bit for bit."""
import numpy as np
import pytest

import medoid_p4_cases as pc
from oracle import c_oracle
from specpride_amd import engine
from test_gpu_fused import _assert_bm_bits, _assert_md_bits, _check, _clean_flags, _md_host
from test_gpu_fused_persistent import fu_grid

pytestmark = pytest.mark.gpu

FUSED = sorted(name for name, (_, fused, _c) in pc.CASES.items() if fused)


@pytest.mark.parametrize("name", FUSED)
def test_p4_through_the_fused_pass(gpu, name):
    csr, facts, _, clean = pc.case(name)
    batch, got, rep, tot = _check(csr, {}, pc.TOL)
    flags = _clean_flags(batch)  # one per parameter set the batch has been run with
    assert flags and set(flags) == {clean}  # completed in the register bodies, or handed on
    if name == "argmin_waves":
        for c, where in facts["where"].items():
            assert rep[c] == csr.cluster_off[c] + where[0]


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_p4_through_medoid_alone(gpu, name):
    csr, facts, _, _ = pc.case(name)
    want = c_oracle.medoid(csr, tol=pc.TOL, with_totals=True)
    batch = engine.DeviceBatch.from_host(csr)
    md = engine.medoid(batch, tolerance=pc.TOL, with_totals=True)
    _assert_md_bits(_md_host(md, csr), want, "oracle")
    # again into the same outputs, and without totals
    md2 = engine.medoid(batch, tolerance=pc.TOL, with_totals=True, out=md)
    _assert_md_bits(_md_host(md2, csr), want, "reused outputs")
    rep = engine.medoid(batch, tolerance=pc.TOL).to_host()
    rep = rep[0] if isinstance(rep, tuple) else rep
    np.testing.assert_array_equal(rep[:csr.n_clusters], want[0])


def test_no_stale_handoff_in_one_workgroup(gpu):
    """One workgroup walks 50, 8, 33, 2, 50, 32, 41 and the two clusters that leave the register
    path between them, in this order: the same bits as on the default grid (and the oracle's)."""
    csr, facts, _, _ = pc.case("stale_handoff")
    batch, got, rep, tot = _check(csr, {}, pc.TOL)
    with fu_grid(1):
        batch1, got1, rep1, tot1 = _check(csr, {}, pc.TOL)
    _assert_bm_bits(got1, got, "one workgroup")
    _assert_md_bits((rep1, tot1), (rep, tot), "one workgroup")
