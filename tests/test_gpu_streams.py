"""The library-owned side stream (round 6, `SideStream` in csrc/spx_api.hip): spx_bin_mean,
spx_gap_average and spx_medoid fork their large clusters' kernels onto it and join it back to the
caller's stream.  Two host threads, each with its own batch and its own HIP stream, call all three
entry points over and over at the same time: every call must give the bits a lone call gives (the
fork/join events are shared per device, so their enqueue must pair up under the lock), and
the caller's stream alone must order the results (they are read after synchronising only
that stream).  (Its first run found a host-side race instead: the packed readback's pinned
staging buffer was one per process; it is one per host thread now.)"""
import threading

import numpy as np
import pytest
import torch

from specpride_amd import engine
from specpride_amd.synthetic import make_clusters_np

pytestmark = pytest.mark.gpu


def _batch_with_giants(seed):
    # clusters past 128 spectra (the bin-mean intake), past 65,536 and 32,768 peaks (the
    # gap-average intake's two tiers), and small ones between them
    sizes = np.array([3, 240, 12, 180, 2, 140, 30, 5] * 3)
    return make_clusters_np(len(sizes), seed=seed, sizes=sizes, n_template=300)


def _digest(res):
    h = res.to_host()
    return [np.asarray(h[k]).tobytes() for k in ("out_off", "out_mz", "out_int", "status", "prec")]


def _medoid_digest(res):
    rep, totals = res.to_host()
    return [rep.tobytes(), totals.tobytes()]


def test_side_stream_concurrent_callers(gpu):
    csrs = [_batch_with_giants(101), _batch_with_giants(102)]
    N = np.diff(csrs[0].spec_off[csrs[0].cluster_off])
    assert (N > 65536).any() and ((N > 32768) & (N <= 65536)).any() and (np.diff(csrs[0].cluster_off) > 128).any()
    batches = [engine.DeviceBatch.from_host(c) for c in csrs]
    want = [(_digest(engine.bin_mean(b)), _digest(engine.gap_average(b))) for b in batches]
    # the third user of the side stream: clusters past MD_NMAX = 64 spectra take medoid's intake
    assert all(engine.medoid_needs_large_path(b) for b in batches)
    want_md = [_medoid_digest(engine.medoid(b, with_totals=True)) for b in batches]
    torch.cuda.synchronize()
    got = [[], []]
    got_md = [[], []]
    errors = []

    def worker(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                bm = engine.bin_mean(batches[i], stream=s)
                ga = engine.gap_average(batches[i], stream=s)
                for _ in range(4):
                    engine.bin_mean(batches[i], out=bm, stream=s)
                    engine.gap_average(batches[i], out=ga, stream=s)
                    md = engine.medoid(batches[i], with_totals=True, stream=s)
                    s.synchronize()  # this stream only
                    got[i].append((_digest(bm), _digest(ga)))
                    got_md[i].append(_medoid_digest(md))
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
    assert not errors, errors
    for i in range(2):
        assert len(got[i]) == 4
        for g in got[i]:
            assert g == want[i]
        assert len(got_md[i]) == 4
        for g in got_md[i]:
            assert g == want_md[i]
