"""The medoid's register tail (medoid_tail_regs, csrc/medoid.hip) on the GPU: every case of
tests/medoid_tail_cases.py through the fused pass (test_gpu_fused._check: the C oracle, the
separate entry points, checked and unchecked, fresh and reused outputs, totals included) and
through engine.medoid alone, bit for bit."""
import numpy as np
import pytest

import medoid_tail_cases as tc
from oracle import c_oracle
from specpride_amd import engine
from test_gpu_fused import _assert_md_bits, _check, _clean_flags, _md_host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_tail_through_the_fused_pass(gpu, name):
    csr, facts, clean = tc.case(name)
    batch, got, rep, tot = _check(csr, {}, tc.TOL)
    assert _clean_flags(batch) == [clean]  # completed in the register bodies, or handed on
    if name == "two_minima":
        c = facts["cluster"]
        assert rep[c] == csr.cluster_off[c] + facts["lo"]
    if name == "identical":
        np.testing.assert_array_equal(rep, csr.cluster_off[:-1])


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_tail_through_medoid_alone(gpu, name):
    csr, facts, clean = tc.case(name)
    want = c_oracle.medoid(csr, tol=tc.TOL, with_totals=True)
    batch = engine.DeviceBatch.from_host(csr)
    md = engine.medoid(batch, tolerance=tc.TOL, with_totals=True)
    _assert_md_bits(_md_host(md, csr), want, "oracle")
    # again into the same outputs, and without totals
    md2 = engine.medoid(batch, tolerance=tc.TOL, with_totals=True, out=md)
    _assert_md_bits(_md_host(md2, csr), want, "reused outputs")
    rep = engine.medoid(batch, tolerance=tc.TOL).to_host()
    rep = rep[0] if isinstance(rep, tuple) else rep
    np.testing.assert_array_equal(rep[:csr.n_clusters], want[0])
