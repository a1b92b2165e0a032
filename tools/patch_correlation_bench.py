#!/usr/bin/env python
"""The patch-correlation weight map (label.fusion.compute_patch_correlation_weight_map) at the size of a cropped thorax: target and atlas phantoms of
256 x 256 x 128 voxels, spacing (0.98, 0.98, 2.5), default parameters (3 mm resampling, 25 mm window).

Times, with HIP events (warm-up first, the two paths alternating inside every repetition),
  * the correlation kernel alone (pp_patch_correlation_f32 on the resampled images) and
  * the whole compute_patch_correlation_weight_map call
against the same map COMPOSED from what the package and torch already offer: smooth_and_resample, then fp64 box sums of t, m,
t^2, m^2, t m and the mask of ones (avg_pool3d over zero-padded tensors), Pearson r from those moments, resample_image, + 1.
The composed map must agree with the kernel's.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import platipy_amd as pa  # noqa: E402
from platipy_amd import runtime  # noqa: E402
from platipy_amd.label import fusion  # noqa: E402
from platipy_amd.registration.utils import resample_image, smooth_and_resample  # noqa: E402


def phantom_pair(size, device):
    """CT-like: -1000 outside an ellipsoidal body of 0 HU with a few organs, 5 HU noise everywhere; the atlas is the same
    anatomy moved by (2, -1, 1) voxels with its own noise."""
    nx, ny, nz = size
    g = torch.Generator(device="cpu").manual_seed(7)
    z, y, x = torch.meshgrid(torch.arange(nz, device=device, dtype=torch.float32), torch.arange(ny, device=device, dtype=torch.float32),
                             torch.arange(nx, device=device, dtype=torch.float32), indexing="ij")

    def inside(c, r):
        return (((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2) < 1.0

    vol = torch.full((nz, ny, nx), -1000.0, device=device)
    body = inside((nx / 2, ny / 2, nz / 2), (0.42 * nx, 0.40 * ny, 0.46 * nz))
    vol[body] = 0.0
    for _ in range(8):
        u = torch.rand(7, generator=g).tolist()
        c = [(0.25 + 0.5 * u[k]) * s for k, s in enumerate((nx, ny, nz))]
        r = [(0.06 + 0.14 * u[3 + k]) * s for k, s in enumerate((nx, ny, nz))]
        vol[inside(c, r) & body] = -200.0 + 600.0 * u[6]
    noise = [torch.randn((nz, ny, nx), generator=g).to(device) * 5.0 for _ in range(2)]
    return (vol + noise[0]).contiguous(), (torch.roll(vol, (1, -1, 2), dims=(0, 1, 2)) + noise[1]).contiguous()


def composed_correlation(t, m, window):
    """Pearson r over the window clipped to the image, from fp64 box sums; 0 where a variance vanishes."""
    wx, wy, wz = window
    pad = ((wx - 1) // 2, wx // 2, (wy - 1) // 2, wy // 2, (wz - 1) // 2, wz // 2)
    volume = float(wx * wy * wz)

    def box(v):
        return F.avg_pool3d(F.pad(v[None, None], pad), (wz, wy, wx), stride=1)[0, 0] * volume

    t, m = t.double(), m.double()
    t, m = t - t.mean(), m - m.mean()          # r does not change; the squares below stay small
    n = box(torch.ones_like(t))
    st, sm = box(t), box(m)
    vt, vm, cov = box(t * t) - st * st / n, box(m * m) - sm * sm / n, box(t * m) - st * sm / n
    den = torch.sqrt(vt.clamp(min=0)) * torch.sqrt(vm.clamp(min=0))
    r = torch.where(den > 0, cov / den, torch.zeros_like(den))
    return r.clamp(-1.0, 1.0).float()


def composed_weight_map(target, moving, p):
    tr = smooth_and_resample(target, isotropic_voxel_size_mm=p["resampled_voxel_size_mm"])
    mr = smooth_and_resample(moving, isotropic_voxel_size_mm=p["resampled_voxel_size_mm"])
    window = [int(p["patch_window_mm"] / s) for s in tr.GetSpacing()]
    return resample_image(tr.like(composed_correlation(tr.tensor, mr.tensor, window)), target) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[256, 256, 128], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "patch_correlation_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "patch_correlation_bench needs a GPU"
    dev = torch.device("cuda", 0)
    spacing = (0.98, 0.98, 2.5)
    tt, tm = phantom_pair(a_.size, dev)
    target, moving = pa.Image(tt, spacing), pa.Image(tm, spacing)
    p = dict(fusion.DEFAULT_VOTE_PARAMS)
    tr = smooth_and_resample(target, isotropic_voxel_size_mm=p["resampled_voxel_size_mm"])
    mr = smooth_and_resample(moving, isotropic_voxel_size_mm=p["resampled_voxel_size_mm"])
    window = [int(p["patch_window_mm"] / s) for s in tr.GetSpacing()]
    ctx = runtime.context(dev)
    corr = torch.empty_like(tr.tensor)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def kernel():
        ctx.patch_correlation(tr.tensor, mr.tensor, tr.GetSize(), window, corr)
        return corr

    cases = {
        "correlation": (kernel, lambda: composed_correlation(tr.tensor, mr.tensor, window)),
        "weight_map": (lambda: fusion.compute_patch_correlation_weight_map(target, moving).tensor,
                               lambda: composed_weight_map(target, moving, p).tensor),
    }
    result = {"size": a_.size, "spacing": spacing, "resampled_size": list(tr.GetSize()),
              "resampled_spacing": [round(s, 6) for s in tr.GetSpacing()], "window": window, "reps": a_.reps}
    for name, (new, old) in cases.items():
        for _ in range(2):                      # warm-up (and the values)
            vn, vo = new().clone(), old()
        diff = float((vn.double() - vo.double()).abs().max())
        assert diff <= 1e-5, (name, diff)
        tn, to = [], []
        for _ in range(a_.reps):
            tn.append(event_ms(new)[0])
            to.append(event_ms(old)[0])
        result[name] = {"new_ms_median": round(statistics.median(tn), 3), "new_ms_min": round(min(tn), 3),
                        "new_ms_spread": round(max(tn) - min(tn), 3), "composed_ms_median": round(statistics.median(to), 3),
                        "composed_ms_min": round(min(to), 3), "composed_ms_spread": round(max(to) - min(to), 3),
                        "composed_over_new": round(statistics.median(to) / statistics.median(tn), 2),
                        "max_abs_difference": diff, "value_min": float(vn.min()), "value_max": float(vn.max())}
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
