"""bench.py's plain line and `--dump-outputs DIR`: a plain run times exactly --steps iterations once and reports nothing
beyond the headline (the rest is --full's), and the dump is the displacement field of the last timed step at a fixed,
seeded sample of voxels -- the same voxels every run, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY_KEYS = ("kernels", "roofline", "roofline_iteration", "kernel_event_pair_ms", "registration_s", "multi_atlas",
                  "multi_atlas_streams", "cpu_baseline")


def _load(d):
    return (np.load(os.path.join(d, "displacement_field_sample.npy")), np.load(os.path.join(d, "displacement_field_sample_index.npy")))


def test_dump_of_a_small_field_is_the_whole_field(tmp_path):
    import bench

    field = torch.arange(3 * 4 * 5 * 6, dtype=torch.float32).reshape(3, 4, 5, 6)
    shapes = bench.dump_outputs(str(tmp_path), field)
    s, i = _load(tmp_path)
    assert s.dtype == np.float32 and i.dtype == np.float64
    assert shapes == {"displacement_field_sample": [3, 120], "displacement_field_sample_index": [120]}
    np.testing.assert_array_equal(i, np.arange(120))
    np.testing.assert_array_equal(s, field.reshape(3, -1).numpy())


def test_dump_of_a_large_field_is_a_fixed_seeded_sample(tmp_path):
    import bench

    field = torch.randn((3, 40, 128, 256), generator=torch.Generator().manual_seed(5))      # 1.3 M voxels > the sample
    nvox = field[0].numel()
    bench.dump_outputs(str(tmp_path / "a"), field)
    bench.dump_outputs(str(tmp_path / "b"), field * 2)
    (sa, ia), (sb, ib) = _load(tmp_path / "a"), _load(tmp_path / "b")
    np.testing.assert_array_equal(ia, ib)                                # the same voxels, whatever the field holds
    assert ia.size == bench.DUMP_SAMPLE_VOXELS
    assert np.all(np.diff(ia) > 0) and ia[0] >= 0 and ia[-1] < nvox and np.all(ia == np.round(ia))
    np.testing.assert_array_equal(sa, field.reshape(3, -1).numpy()[:, ia.astype(np.int64)])
    np.testing.assert_array_equal(sb, 2 * sa)
    total = sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20


def test_bench_offers_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_plain_bench_line_and_dump(tmp_path):
    """`bench.py --steps 3 --warmup 1 --dump-outputs DIR` on the 512 x 512 x 256 pair: one timed block of 3 steps, the headline keys
    only, and a finite, non-zero field sample on disk."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "PP_BENCH_STUB")}
    out_dir = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["metric"] == "Mvoxels/s per demons iter, 512x512x256 fp32" and r["unit"] == "Mvoxels/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["steps"] == 3 and r["warmup"] == 1 and r["full"] is False and r["repeats"]["n"] == 1
    assert r["ms_per_step"] > 0 and abs(r["value"] - 512 * 512 * 256 / (r["ms_per_step"] * 1e3)) <= 1e-6 * r["value"]
    assert not [k for k in FULL_ONLY_KEYS if k in r], r.keys()
    s, i = _load(out_dir)
    assert s.shape == (3, i.size) and np.isfinite(s).all() and np.abs(s).max() > 0
