"""The fused pass's persistent loop (bin_mean_medoid_kernel, csrc/fused.hip): state that
crosses cluster boundaries.

One workgroup walks many clusters: it claims them from a queue head in the bin-mean
workspace, keeps the next cluster's header in a second LDS buffer while the current one is
processed, and reuses the LDS union from cluster to cluster.  The single-cluster edges are
tests/test_gpu_fused.py's; here the batches of tests/fused_sequences.py (whose properties
tests/test_fused_sequences_inputs.py proves on the host) put every kind of cluster next to
every other, under grids capped by SPX_FU_GRID so that few workgroups walk many clusters,
and each goes through test_gpu_fused._check: the C oracle and the separate entry points,
checked and unchecked, fresh and reused outputs.
"""
import os

import numpy as np
import pytest

import fused_sequences as fs
from oracle import c_oracle
from specpride_amd import engine
from test_gpu_fused import _assert_bm_bits, _assert_md_bits, _check, _md_host

pytestmark = pytest.mark.gpu


class fu_grid:
    """SPX_FU_GRID for the calls inside the block (None: the default grid)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("SPX_FU_GRID", None)
        if self.value is not None:
            os.environ["SPX_FU_GRID"] = str(self.value)

    def __exit__(self, *exc):
        os.environ.pop("SPX_FU_GRID", None)
        if self.old is not None:
            os.environ["SPX_FU_GRID"] = self.old


def test_one_small_cluster_default_grid(gpu):
    """C = 1: one workgroup, one claim that finds a cluster and one that ends the loop."""
    _check(fs.ordinary_batch(1), {}, fs.TOL)


@pytest.mark.parametrize("grid", [1, 2, 3, None])
def test_every_ordered_pair_of_kinds(gpu, grid):
    """Every kind of cluster directly after every kind, itself included: with one workgroup
    in the sequence's own order, with 2 and 3 in the orders their claims interleave to, and
    on the default grid (a workgroup per cluster at this size)."""
    csr, names = fs.sequence()
    with fu_grid(grid):
        batch, got, rep, tot = _check(csr, {}, fs.TOL)
    assert np.all(rep[np.diff(csr.cluster_off) > 0] >= 0)


@pytest.mark.parametrize("C", [3, 4, 5, 9])
def test_grid_edges(gpu, C):
    """A grid of 4 over 3, 4, 5 and 9 clusters: fewer clusters than workgroups (the grid
    is capped at C), exactly as many, one more, and more than twice as many."""
    with fu_grid(4):
        _check(fs.ordinary_batch(C), {}, fs.TOL)


@pytest.mark.parametrize("grid", [2, None])
def test_every_cluster_exactly_once(gpu, grid):
    """Outputs poisoned before the call: no sentinel survives in status, count or rep, so
    every cluster was claimed; a second call on the same workspace gives the same bits, so
    the queue head was zeroed again and no cluster was claimed twice into another's place."""
    import torch

    csr, names = fs.sequence()
    ref = c_oracle.bin_mean(csr)
    ref_rep, ref_tot = c_oracle.medoid(csr, tol=fs.TOL, with_totals=True)
    batch = engine.DeviceBatch.from_host(csr)
    C = csr.n_clusters
    with fu_grid(grid):
        bm, md = engine.bin_mean_medoid(batch, tolerance=fs.TOL, with_totals=True)
        for call in range(2):
            bm.status.fill_(-77)
            bm.count.fill_(-77)
            md.rep.fill_(-77)
            md.totals.fill_(float("nan"))
            engine.bin_mean_medoid(batch, tolerance=fs.TOL, out_bm=bm, out_md=md)
            torch.cuda.synchronize()
            assert not (bm.status[:C] == -77).any().item(), f"call {call}: a status was never written"
            assert not (bm.count[:C] == -77).any().item(), f"call {call}: a count was never written"
            assert not (md.rep[:C] == -77).any().item(), f"call {call}: a representative was never written"
            got = bm.to_host()
            for k in ("status", "out_off", "out_mz", "out_int"):
                np.testing.assert_array_equal(got[k], ref[k], err_msg=f"call {call}: {k}")
            rep, tot = _md_host(md, csr)
            _assert_md_bits((rep, tot), (ref_rep, ref_tot), f"call {call}")


def test_two_streams_at_once(gpu):
    """Two batches on two streams at the same time, each with its own workspace (its own
    queue head): both equal their serial results."""
    import torch

    a_csr, _ = fs.sequence()
    b_csr = fs.ordinary_batch(64, seed=301)
    serial = []
    for csr in (a_csr, b_csr):
        bm, md = engine.bin_mean_medoid(engine.DeviceBatch.from_host(csr), tolerance=fs.TOL, with_totals=True)
        serial.append((bm.to_host(), _md_host(md, csr)))
    torch.cuda.synchronize()
    batches = [engine.DeviceBatch.from_host(csr) for csr in (a_csr, b_csr)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with fu_grid(3):  # few workgroups each, so both kernels are resident together
        outs = [engine.bin_mean_medoid(b, tolerance=fs.TOL, with_totals=True) for b in batches]  # workspaces made
        torch.cuda.synchronize()
        for _ in range(2):
            for b, s, (bm, md) in zip(batches, streams, outs):
                engine.bin_mean_medoid(b, tolerance=fs.TOL, out_bm=bm, out_md=md, stream=s, check=False)
        for s in streams:
            s.synchronize()
    for csr, (bm, md), (want_bm, want_md) in zip((a_csr, b_csr), outs, serial):
        _assert_bm_bits(bm.to_host(), want_bm, "two streams")
        _assert_md_bits(_md_host(md, csr), want_md, "two streams")
