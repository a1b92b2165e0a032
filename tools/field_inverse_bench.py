#!/usr/bin/env python
"""Displacement-field inversion and Jacobian determinant at the size of a planning CT: a 512 x 512 x 256 field, spacing
(0.98, 0.98, 2.5), smooth, 6 mm at its largest and zero near the border.

Times, with HIP events (warm-up first, the paths alternating inside every repetition, medians of --reps),
  * ten iterations of pa.registration.invert_displacement_field with both thresholds at 0 (pp_invert_field_f32: one launch per
    iteration, 60 B per voxel and iteration -- v and the kept residual read and written, one compulsory gather of u --, no host
    read in between) against the same ten iterations composed from torch.nn.functional.grid_sample and elementwise ops, with M
    kept on the device;
  * pa.registration.displacement_field_jacobian_determinant with and without its statistics (pp_jacobian_determinant_f32:
    16 B per voxel) against a composition of torch slices on a replicate-padded field.
The two paths' results are compared in the same run (the largest difference is reported and has to stay below what the torch
path's fp32 normalised coordinates allow).  Prints one JSON line; --out writes it to a file."""
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

INVERT_BYTES_PER_VOXEL_ITERATION = 60
JACOBIAN_BYTES_PER_VOXEL = 16


def smooth_field(size, spacing, dev):
    nx, ny, nz = size
    ctx = runtime.context(dev)
    field = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=dev)
    lat = field[:, 16:-16:16, 32:-32:32, 32:-32:32]
    lat.copy_(torch.randn(tuple(lat.shape), generator=torch.Generator().manual_seed(3)).to(dev))
    ctx.recursive_gaussian_field(field, pa.Image(field, spacing, is_vector=True).geom(), [12.0, 12.0, 12.0])
    field *= 6.0 / float(field.abs().max())
    z, y, x = (torch.arange(n, device=dev, dtype=torch.float32) for n in (nz, ny, nx))
    win = [torch.clamp(torch.minimum(i, (n - 1) - i) / 8.0, max=1.0) for i, n in ((z, nz), (y, ny), (x, nx))]
    field *= win[0].view(-1, 1, 1) * win[1].view(1, -1, 1) * win[2].view(1, 1, -1)
    return field.contiguous()


def torch_invert(u, spacing, iterations):
    """The same iteration from grid_sample (border padding = the clamped interpolation) and elementwise ops."""
    _, nz, ny, nx = u.shape
    dev = u.device
    sp = torch.tensor(spacing, device=dev, dtype=torch.float32).view(3, 1, 1, 1)
    z, y, x = torch.meshgrid(torch.arange(nz, device=dev, dtype=torch.float32), torch.arange(ny, device=dev, dtype=torch.float32),
                             torch.arange(nx, device=dev, dtype=torch.float32), indexing="ij")
    idx = torch.stack([x, y, z])
    n = torch.tensor([nx, ny, nz], device=dev, dtype=torch.float32).view(3, 1, 1, 1)
    border = (idx == 0).any(0) | (idx == n - 1).any(0)
    v = torch.zeros_like(u)
    for k in range(1, iterations + 1):
        c = idx + v / sp
        inside = ((c >= -0.5) & (c < n - 0.5)).all(0)
        grid = (2.0 * c / (n - 1) - 1.0).permute(1, 2, 3, 0).unsqueeze(0)
        samp = F.grid_sample(u.unsqueeze(0), grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
        r = -(v + samp * inside)
        s = torch.sqrt(((r / sp) ** 2).sum(0))
        eps = 0.75 if k == 1 else 0.5
        lim = eps * s.max()                      # stays on the device
        v = v + eps * r * torch.where(s > lim, lim / s, torch.ones_like(s))
        v[:, border] = 0.0
    return v


def torch_jacobian(u, spacing):
    p = F.pad(u.unsqueeze(0), (1, 1, 1, 1, 1, 1), mode="replicate")[0]
    w = [0.5 / s for s in spacing]
    gx = w[0] * (p[:, 1:-1, 1:-1, 2:] - p[:, 1:-1, 1:-1, :-2])
    gy = w[1] * (p[:, 1:-1, 2:, 1:-1] - p[:, 1:-1, :-2, 1:-1])
    gz = w[2] * (p[:, 2:, 1:-1, 1:-1] - p[:, :-2, 1:-1, 1:-1])
    J = [[g[j] + (1.0 if i == j else 0.0) for j in range(3)] for i, g in enumerate((gx, gy, gz))]
    return (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
            + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "field_inverse_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "field_inverse_bench needs a GPU"
    dev = torch.device("cuda", 0)
    spacing = (0.98, 0.98, 2.5)
    u = smooth_field(a_.size, spacing, dev)
    field = pa.Image(u, spacing, is_vector=True)
    nvox = u[0].numel()
    its = a_.iterations

    def hip_invert():
        return pa.registration.invert_displacement_field(field, its, 0.0, 0.0)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for _ in range(2):      # warm-up, and the values
        got, want = hip_invert().tensor, torch_invert(u, spacing, its)
    sp = torch.tensor(spacing, device=dev).view(3, 1, 1, 1)
    inv_diff = float(torch.sqrt((((got - want) / sp) ** 2).sum(0)).max())
    _, info = pa.registration.invert_displacement_field(field, its, 0.0, 0.0, return_info=True)
    # grid_sample forms its sample position from an fp32 coordinate normalised to [-1, 1]: 2^-24 of 512 voxels is 3e-5 voxel,
    # through ten iterations of a field with neighbour differences well below 1
    assert inv_diff < 1e-2, f"the two inversions differ by {inv_diff} voxel"
    del got, want
    th, tt = [], []
    for _ in range(a_.reps):
        th.append(event_ms(hip_invert)[0])
        tt.append(event_ms(lambda: torch_invert(u, spacing, its))[0])

    def hip_jac():
        return pa.registration.displacement_field_jacobian_determinant(field)

    def hip_jac_stats():
        return pa.registration.displacement_field_jacobian_determinant(field, return_stats=True)

    for _ in range(2):
        jd, jt = hip_jac().tensor, torch_jacobian(u, spacing)
    jac_diff = float((jd - jt).abs().max())
    assert jac_diff < 1e-4, f"the two determinants differ by {jac_diff}"
    _, stats = hip_jac_stats()
    assert stats["min"] == float(jd.min()) and stats["max"] == float(jd.max()) and stats["count"] == nvox
    del jd, jt
    tj, tjs, tjt = [], [], []
    for _ in range(a_.reps):
        tj.append(event_ms(hip_jac)[0])
        tjs.append(event_ms(hip_jac_stats)[0])
        tjt.append(event_ms(lambda: torch_jacobian(u, spacing))[0])
    mh, mt, mj, mjs, mjt = (statistics.median(t) for t in (th, tt, tj, tjs, tjt))

    def spread(t):
        return round(max(t) - min(t), 3)

    result = {"size": a_.size, "spacing": spacing, "iterations": its, "reps": a_.reps, "field_abs_max_mm": round(float(u.abs().max()), 2),
              "structure": "residual kept in scratch, one gather per iteration",
              "invert_ms_median": round(mh, 3), "invert_ms_spread": spread(th), "invert_ms_per_iteration": round(mh / its, 3),
              "invert_bytes_per_voxel_iteration": INVERT_BYTES_PER_VOXEL_ITERATION,
              "invert_GB_per_s": round(INVERT_BYTES_PER_VOXEL_ITERATION * nvox * its / (mh * 1e-3) / 1e9, 1),
              "torch_invert_ms_median": round(mt, 3), "torch_invert_ms_spread": spread(tt), "torch_over_hip_invert": round(mt / mh, 2),
              "invert_max_difference_voxel": inv_diff, "invert_last_max_error_norm": info["max_error_norm"],
              "invert_last_mean_error_norm": info["mean_error_norm"],
              "jacobian_ms_median": round(mj, 3), "jacobian_ms_spread": spread(tj),
              "jacobian_GB_per_s": round(JACOBIAN_BYTES_PER_VOXEL * nvox / (mj * 1e-3) / 1e9, 1),
              "jacobian_stats_ms_median": round(mjs, 3), "jacobian_stats_ms_spread": spread(tjs),
              "jacobian_stats_GB_per_s": round(JACOBIAN_BYTES_PER_VOXEL * nvox / (mjs * 1e-3) / 1e9, 1),
              "torch_jacobian_ms_median": round(mjt, 3), "torch_jacobian_ms_spread": spread(tjt), "torch_over_hip_jacobian": round(mjt / mj, 2),
              "jacobian_max_difference": jac_diff, "jacobian_min": stats["min"], "jacobian_count_nonpositive": stats["count_nonpositive"]}
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
