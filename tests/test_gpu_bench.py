"""bench.py on the GPU at a small size: what a plain run prints and leaves out, what
``--dump-outputs`` writes, and that ``--full`` still brings the other lines.

Two plain runs with the same arguments (one module fixture) must write identical files;
the files must be what a caller of the timed path receives, so they are compared with the
two separate entry points run here on the same seeded batch (bit for bit, as the fused
pass is defined: DESIGN.md §6)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from specpride_amd import engine
from specpride_amd.csr import concat_ranges
from specpride_amd.synthetic import make_clusters_torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTERS, SEED, STEPS = 300, 5, 3
FULL_ONLY = ("roofline", "roofline_bin_mean", "roofline_medoid", "kernels", "separate_step", "gap_average",
             "config3_medoid", "bin_mean_shapes", "medoid_shapes", "gap_average_shapes", "tier2_host_inclusive",
             "tier3_mgf_to_mgf", "north_star_1m", "cpu_baseline", "cpu_baseline_all_cores")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SPX_BENCH_BACKEND", "SPX_BENCH_REHEARSE")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--clusters", str(CLUSTERS),
                        "--seed", str(SEED), "--steps", str(STEPS), "--warmup", "1", *argv],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain_runs(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("bench_dump")
    dirs = [str(root / "a"), str(root / "b")]
    return [_bench("--dump-outputs", d) for d in dirs], dirs


def test_plain_line_is_the_headline_alone(plain_runs):
    (d, _), _ = plain_runs
    assert d["metric"] == "clusters/sec (whole node) for medoid + binned consensus"
    assert d["unit"] == "clusters/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["n_gpus"] == 1 and d["steps"] == STEPS and d["warmup"] == 1
    assert d["ms_per_step"] > 0
    # value is the batch's clusters over the mean timed step (both rounded in the line)
    assert d["value"] == pytest.approx(CLUSTERS / (d["ms_per_step"] * 1e-3), rel=1e-2)
    assert not [k for k in FULL_ONLY if k in d]


def test_dump_is_repeatable_and_bounded(plain_runs):
    _, (a, b) = plain_runs
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert set(names) == {n + ".npy" for n in ("rep", "count", "status", "prec", "charge", "sample_ids",
                                                "sample_off", "out_mz", "out_int")}
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64)
        assert x.tobytes() == y.tobytes(), n
        total += os.path.getsize(os.path.join(a, n))
    assert total <= 64_000_000


def test_dump_is_what_the_entry_points_return(plain_runs, gpu):
    _, (a, _) = plain_runs
    got = {n[:-4]: np.load(os.path.join(a, n)) for n in os.listdir(a)}
    batch = engine.DeviceBatch.from_device(make_clusters_torch(CLUSTERS, seed=SEED, device=gpu))
    h = engine.bin_mean(batch).to_host()
    rep, _ = engine.medoid(batch).to_host()
    cnt = np.diff(h["out_off"])
    np.testing.assert_array_equal(got["rep"], rep[:CLUSTERS])
    np.testing.assert_array_equal(got["count"], cnt)
    np.testing.assert_array_equal(got["status"], h["status"])
    np.testing.assert_array_equal(got["prec"], h["prec"])
    np.testing.assert_array_equal(got["charge"], h["charge"])
    ids = got["sample_ids"].astype(np.int64)
    assert len(ids) == CLUSTERS and np.array_equal(ids, np.arange(CLUSTERS))  # fewer clusters than the sample cap
    np.testing.assert_array_equal(np.diff(got["sample_off"]), cnt[ids])
    sel = concat_ranges(h["out_off"][ids], cnt[ids])
    assert got["out_mz"].tobytes() == h["out_mz"][sel].tobytes()
    assert got["out_int"].tobytes() == h["out_int"][sel].tobytes()


def test_full_adds_the_kernel_lines(gpu):
    d = _bench("--full", "--no-extras", "--no-cpu-baseline")
    assert d["steps"] == STEPS and d["ms_per_step"] > 0
    for k in ("roofline", "roofline_bin_mean", "roofline_medoid", "kernels"):
        assert k in d
    assert d["roofline"]["kernel"] == "bin_mean_medoid_kernel"
