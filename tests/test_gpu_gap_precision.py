"""Gap-average group sums against EXACT arithmetic under a wide dynamic range, on every
code path of the chain (tests/test_gap_precision_inputs.py builds the inputs, proves them
fair on the CPU and lists what is out of scope).

One contract for every path and spike level:

* the status equals the oracle's;
* below the spike's m/z the emitted groups are exactly the exact kept set, both columns
  within GAP_RTOL of the exact values AND of the C oracle (which has not met the spike there);
* the whole cluster, for every level but the 1e300 one: the emitted set is the exact kept
  set, values within GAP_RTOL of exact -- and assert_gap_close against the C oracle where
  the oracle itself is that accurate (reference-comparable clusters);
* above a 1e300 spike the reference loses every group (cumsum differences of 0.0 or
  inf - inf), so only finite or reference-identical values are required there.

GAP_RTOL is the project's published bar (1e-9), imported, not re-derived.

Which kernel serves a shape is pinned on the CPU (test_shape_lands_on_its_path: the peak
counts and m/z spans that the chain branches on); the profiler names only the LDS and wide
kernels, each launched once per call whatever the batch.  A cluster whose one scale per
cluster is too coarse is handed down the chain, so the lds and wide spike cases are answered
by the global kernel's per-group sums, and the giant ones by the giant pipeline's last step.
No case is skipped or expected to fail."""
import numpy as np
import pytest

from oracle import c_oracle
from specpride_amd import _lib, engine
from specpride_amd.csr import SpectraCSR
from test_gap_precision_inputs import (CASES, EXTRA_CASES, LEVELS, PARAM_SETS, _params, case, cluster_values,
                                       reference_comparable, references, rel_err, split_at_spike)
from test_gpu_parity import GAP_RTOL, assert_bin_mean_equal, assert_gap_close

pytestmark = pytest.mark.gpu


def _gap(csr, pi, profile=False):
    batch = engine.DeviceBatch.from_host(csr)
    if profile:
        _lib.profile_enable(True)
    try:
        got = engine.gap_average(batch, **_params(PARAM_SETS[pi])).to_host()
        launches = {k: _lib.profile_read(k)[1] for k in ("gap_average_lds_kernel", "gap_average_wide_kernel")} \
            if profile else None
    finally:
        if profile:
            _lib.profile_enable(False)
    return got, launches


def _report(tag, **figs):
    print("GAPPREC", tag, " ".join(f"{k}={v:.2e}" for k, v in figs.items()))


def _check(tag, csr, got, ex, ref, pi, whole, comparable, level):
    """The contract above for every cluster of one result; figures printed before any assertion."""
    figs = dict(below_exact=0.0, below_ref=0.0, whole_exact=0.0)
    for c in range(csr.n_clusters):
        sp = csr.spike_mz[c]
        (gb, ga), (eb, ea), (rb, _) = (split_at_spike(*cluster_values(r, c), sp) for r in (got, ex, ref))
        figs["below_exact"] = max(figs["below_exact"], rel_err(gb[0], eb[0]), rel_err(gb[1], eb[1]))
        figs["below_ref"] = max(figs["below_ref"], rel_err(gb[0], rb[0]), rel_err(gb[1], rb[1]))
        gm, gi = cluster_values(got, c)
        em, ei = cluster_values(ex, c)
        figs["whole_exact"] = max(figs["whole_exact"], rel_err(gm, em), rel_err(gi, ei))
    _report(tag, **figs)
    np.testing.assert_array_equal(got["status"], ref["status"])
    for c in range(csr.n_clusters):
        sp = csr.spike_mz[c]
        (gb, ga), (eb, ea), (rb, ra) = (split_at_spike(*cluster_values(r, c), sp) for r in (got, ex, ref))
        for k, name in ((0, "m/z"), (1, "intensity")):
            assert len(gb[k]) == len(eb[k]), f"{tag} cluster {c}: {len(gb[k])} groups below the spike, exact {len(eb[k])}"
            np.testing.assert_allclose(gb[k], eb[k], rtol=GAP_RTOL, atol=0, err_msg=f"{tag} cluster {c} {name} vs exact")
            np.testing.assert_allclose(gb[k], rb[k], rtol=GAP_RTOL, atol=0, err_msg=f"{tag} cluster {c} {name} vs oracle")
        if whole:
            for k, name in ((0, "m/z"), (1, "intensity")):
                assert len(ga[k]) == len(ea[k]), f"{tag} cluster {c}: {len(ga[k])} groups above the spike, exact {len(ea[k])}"
                np.testing.assert_allclose(ga[k], ea[k], rtol=GAP_RTOL, atol=0,
                                           err_msg=f"{tag} cluster {c} {name} above the spike vs exact")
        elif all(rel_err(ga[k], ea[k]) <= GAP_RTOL for k in (0, 1)):
            pass  # the exact values (with the non-finite shape's NaN m/z in the last group)
        elif not (np.isfinite(ga[0]).all() and np.isfinite(ga[1]).all()):
            np.testing.assert_array_equal(ga[0], ra[0])
            np.testing.assert_array_equal(ga[1], ra[1])
    if whole and comparable:
        assert_gap_close(got, ref, _params(PARAM_SETS[pi])["dyn_range"])


@pytest.mark.parametrize("path,level", CASES)
def test_gap_sums_under_a_discarded_spike(gpu, path, level):
    csr = case(path, level)
    for pi in range(len(PARAM_SETS)):
        ex, ref = references(path, level, pi)
        got, launches = _gap(csr, pi, profile=True)
        # one launch of each per call for EVERY shape: this pins the call's shape, not the path taken
        assert launches == {"gap_average_lds_kernel": 1, "gap_average_wide_kernel": 1}
        comparable = all(reference_comparable(path, level, pi, c) for c in range(csr.n_clusters))
        _check(f"{path} {level} dyn={_params(PARAM_SETS[pi])['dyn_range']:g}", csr, got, ex, ref, pi,
               whole=LEVELS[level] is not None, comparable=comparable, level=level)


@pytest.mark.parametrize("path,level,kept,outlier", EXTRA_CASES)
def test_gap_sums_kept_spike_and_mz_outliers(gpu, path, level, kept, outlier):
    """A kept spike (the group sets gmax, the filter removes most others): the whole cluster
    against exact.  An m/z outlier (1e9, 1e12: the last true group, merged into the last
    emitted one): every group but the last emitted one."""
    csr = case(path, level, kept, outlier)
    for pi in range(len(PARAM_SETS)):
        ex, ref = references(path, level, pi, kept, outlier)
        got, _ = _gap(csr, pi)
        tag = f"{path} {'kept ' + level if kept else f'outlier {outlier:g}'} dyn={_params(PARAM_SETS[pi])['dyn_range']:g}"
        worst = 0.0
        for c in range(csr.n_clusters):
            (gm, gi), (em, ei) = cluster_values(got, c), cluster_values(ex, c)
            if outlier is not None and len(gm) and len(em):
                gm, gi, em, ei = gm[:-1], gi[:-1], em[:-1], ei[:-1]
            worst = max(worst, rel_err(gm, em), rel_err(gi, ei))
        _report(tag, whole_exact=worst)
        np.testing.assert_array_equal(got["status"], ref["status"])
        for c in range(csr.n_clusters):
            (gm, gi), (em, ei) = cluster_values(got, c), cluster_values(ex, c)
            assert len(gm) == len(em), f"{tag} cluster {c}: {len(gm)} groups, exact {len(em)}"
            if outlier is not None:
                gm, gi, em, ei = gm[:-1], gi[:-1], em[:-1], ei[:-1]
            np.testing.assert_allclose(gm, em, rtol=GAP_RTOL, atol=0, err_msg=f"{tag} cluster {c} m/z")
            np.testing.assert_allclose(gi, ei, rtol=GAP_RTOL, atol=0, err_msg=f"{tag} cluster {c} intensity")


@pytest.mark.parametrize("path", ["lds", "wide", "giant_intake"])
def test_gap_average_scales_with_powers_of_two(gpu, path):
    """Every intensity times 2^600 and 2^-600: offsets and m/z bitwise unchanged, intensities
    bitwise the original ones times the same power (the reference has the same property on
    these inputs: test_reference_scales_with_powers_of_two)."""
    csr = case(path, "1e6")
    for pi in range(len(PARAM_SETS)):
        base, _ = _gap(csr, pi)
        for e in (600, -600):
            scaled = SpectraCSR(csr.cluster_off, csr.spec_off, csr.mz, np.ldexp(csr.inten, e), csr.prec_mz,
                                csr.charge, csr.rt)
            got, _ = _gap(scaled, pi)
            np.testing.assert_array_equal(got["status"], base["status"])
            np.testing.assert_array_equal(got["out_off"], base["out_off"])
            np.testing.assert_array_equal(got["out_mz"].view(np.int64), base["out_mz"].view(np.int64))
            np.testing.assert_array_equal(got["out_int"].view(np.int64), np.ldexp(base["out_int"], e).view(np.int64))


@pytest.mark.parametrize("path", ["lds", "wide", "global", "giant_global", "giant_intake"])
@pytest.mark.parametrize("level", list(LEVELS))
def test_bin_mean_bit_exact_on_spiky_batches(gpu, path, level):
    """The same batches through bin-mean (one call, staged, and fused with the medoid):
    summation order matters most under a spike, so the bit-exact claim is pinned here.
    (Not the non-finite shape: it differs from the lds one by a NaN m/z, which bin-mean's
    range test drops before any sum -- the nonfinite goldens pin that.)"""
    csr = case(path, level)
    ref = c_oracle.bin_mean(csr)
    batch = engine.DeviceBatch.from_host(csr)
    assert_bin_mean_equal(engine.bin_mean(batch).to_host(), ref)
    assert_bin_mean_equal(engine.bin_mean(batch, staged=True).to_host(), ref)
    bm, md = engine.bin_mean_medoid(batch)
    assert_bin_mean_equal(bm.to_host(), ref)
    rep, _ = md.to_host()
    np.testing.assert_array_equal(rep[:csr.n_clusters], c_oracle.medoid(csr))
