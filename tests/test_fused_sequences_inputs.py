"""The persistent loop's inputs (tests/fused_sequences.py): proof that they are what they claim.

No GPU here.  Every kind's named property is asserted on the host with the helpers of
tests/fused_cases.py, the sequence is shown to hold every ordered pair of kinds, and the two
oracles are shown to agree on it, which is the anchor tests/test_gpu_fused_persistent.py
leans on.
"""
import numpy as np
import pytest

import fused_cases as fc
import fused_sequences as fs
from oracle import c_oracle, np_oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _descents(mz):
    """Indices i with mz[i] > mz[i + 1] (NaN compares false)."""
    return np.flatnonzero(mz[:-1] > mz[1:])


def _plain(csr, c=0):
    """Sorted, finite, one charge."""
    s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
    ok = len(set(csr.charge[s0:s1])) == 1
    for s in range(s0, s1):
        mz = csr.spectrum(s)[0]
        ok = ok and np.all(np.isfinite(mz)) and len(_descents(mz)) == 0
    return bool(ok)


@pytest.mark.parametrize("name", ["n2", "n50_full", "n1"])
def test_kinds_the_register_bodies_complete(name):
    csr = fs.kind_csr(name)
    n = {"n2": 2, "n50_full": fc.BR_NMAX, "n1": 1}[name]
    assert csr.n_clusters == 1 and csr.n_spectra == n
    assert _plain(csr) and fc.fits_register_path(csr, 0, tol=fs.TOL)


def test_n50_full_fills_both_bodies():
    csr = fs.kind_csr("n50_full")
    D, K = fc.cluster_D(csr, 0), fc.cluster_K(csr, 0, fs.TOL)
    assert fc.BM_DCAP - 16 < D <= fc.BM_DCAP                   # "D near 1,536"
    assert fc.MD_KMAX - 16 < K <= fc.MD_KMAX                   # "K near 1,728"
    assert ((K + 63) // 64 | 1) == fc.MD_KWMAX                 # every row word in use
    lens = fc.spectrum_lengths(csr, 0)
    assert lens.min() >= 30 and lens.max() <= fc.BM_FASTLEN
    tot = np_oracle.medoid_cluster([m for m, _ in csr.cluster(0)], fs.TOL)[1]
    assert len(np.unique(tot)) > 1                             # the distances differ


def test_kinds_not_here():
    a, b = fs.kind_csr("n51"), fs.kind_csr("len253")
    assert a.n_spectra == fc.BR_NMAX + 1 and _plain(a)
    assert fc.spectrum_lengths(a, 0).max() <= fc.BM_FASTLEN
    assert b.n_spectra <= fc.BR_NMAX and _plain(b)
    assert sorted(fc.spectrum_lengths(b, 0))[-2:] == [126, fc.BM_FASTLEN + 1]


def test_kind_mixed_charge():
    csr = fs.kind_csr("mixed_charge")
    assert sorted(set(csr.charge)) == [2, 3] and csr.n_spectra <= fc.BR_NMAX
    assert c_oracle.bin_mean(csr)["out_off"][-1] == 0          # nothing emitted


def test_kinds_deferred_at_the_vote():
    inv, nan = fs.kind_csr("inversion"), fs.kind_csr("nan_mz")
    for csr in (inv, nan):
        assert csr.n_spectra <= fc.BR_NMAX and fc.spectrum_lengths(csr, 0).max() <= fc.BM_FASTLEN
        assert len(set(csr.charge)) == 1
    # exactly one descent in the whole cluster, both peaks in range, in different bins
    where = [(s, i) for s in range(inv.n_spectra) for i in _descents(inv.spectrum(s)[0])]
    assert len(where) == 1 and np.all(np.isfinite(inv.mz))
    s, i = where[0]
    pair = inv.spectrum(s)[0][i:i + 2]
    assert np.all(fc.in_range(pair)) and len(set(fc.bin_mean_bins(pair))) == 2
    assert np.count_nonzero(np.isnan(nan.mz)) == 1
    assert all(len(_descents(nan.spectrum(s)[0])) == 0 for s in range(nan.n_spectra))


def test_kinds_over_a_cap():
    d, k = fs.kind_csr("d_over"), fs.kind_csr("k_over")
    assert _plain(d) and fc.cluster_D(d, 0) == fc.BM_DCAP + 1
    assert fc.cluster_K(d, 0, fs.TOL) <= fc.MD_KMAX             # only the bin-mean's cap is passed
    assert _plain(k) and fc.cluster_K(k, 0, fs.TOL) == fc.MD_KMAX + 1
    assert fc.cluster_D(k, 0) <= fc.BM_DCAP                     # only the medoid's
    for csr in (d, k):
        assert csr.n_spectra <= fc.BR_NMAX and fc.spectrum_lengths(csr, 0).max() <= fc.BM_FASTLEN


def test_kind_md_out():
    csr = fs.kind_csr("md_out")
    bins = np_oracle.xcorr_bins(fc.cluster_mz(csr, 0), fs.TOL)
    assert bins.max() == fc.MD_BINS and bins.min() >= 0
    assert _plain(csr) and fc.cluster_D(csr, 0) <= fc.BM_DCAP and csr.n_spectra <= fc.BR_NMAX


def test_kind_all_out():
    csr = fs.kind_csr("all_out")
    assert _plain(csr) and not fc.in_range(csr.mz).any() and fc.cluster_D(csr, 0) == 0
    assert fc.cluster_K(csr, 0, fs.TOL) > 1 and csr.n_spectra >= 2


def test_pair_walk_is_an_euler_circuit():
    for k in (1, 2, 3, 5, len(fs.KINDS)):
        w = fs.pair_walk(k)
        assert len(w) == k * k + 1 and w[0] == w[-1]
        assert set(zip(w[:-1], w[1:])) == {(a, b) for a in range(k) for b in range(k)}


def test_sequence_holds_every_ordered_pair():
    csr, names = fs.sequence()
    k = len(fs.KINDS)
    assert 10 <= k and csr.n_clusters == len(names) == k * k + 1
    assert set(zip(names[:-1], names[1:])) == {(a, b) for a in fs.KINDS for b in fs.KINDS}
    # cluster c IS its kind's cluster
    for c in (0, 1, len(names) // 2, len(names) - 1):
        one = fs.kind_csr(names[c])
        np.testing.assert_array_equal(_bits(fc.cluster_mz(csr, c)), _bits(one.mz))
    sizes = np.diff(csr.cluster_off)
    assert sizes.max() == fc.BR_NMAX + 1 and np.diff(csr.spec_off).max() == fc.BM_FASTLEN + 1


def test_oracles_agree_on_the_sequence():
    csr, _ = fs.sequence()
    a, b = c_oracle.bin_mean(csr), np_oracle.bin_mean(csr)
    for k in ("status", "out_off", "charge"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in ("out_mz", "out_int", "prec"):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
    rep, tot = c_oracle.medoid(csr, tol=fs.TOL, with_totals=True)
    for name in fs.KINDS:
        c = fs.sequence()[1].index(name)
        s0, s1 = csr.cluster_off[c], csr.cluster_off[c + 1]
        k, t = np_oracle.medoid_cluster([m for m, _ in csr.cluster(c)], fs.TOL)
        np.testing.assert_array_equal(_bits(tot[s0:s1]), _bits(t), err_msg=name)
        assert rep[c] == s0 + int(np.flatnonzero(t == t.min())[0]), name


def test_ordinary_batches_stay_in_the_register_bodies():
    for C in (1, 3, 4, 5, 9):
        csr = fs.ordinary_batch(C)
        assert csr.n_clusters == C
        assert all(fc.fits_register_path(csr, c, tol=fs.TOL) for c in range(C))
