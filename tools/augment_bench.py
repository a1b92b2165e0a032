#!/usr/bin/env python
"""Deformable augmentation at the size of a planning CT: a 512 x 512 x 256 fp32 image, spacing (0.98, 0.98, 2.5), 8 uint8
ellipsoid structures and one smoothed displacement field.

Times, with HIP events (warm-up first, the two paths alternating inside every repetition, medians),
  * pa.registration.apply_transform_to_set -- the image (linear) and the 8 structures through the field in ONE gather
    (pp_resample_set) -- against
  * the same nine outputs from nine pa.registration.apply_transform calls (pp_resample_f32 / pp_resample_u8, the path
    without the fused call),
after asserting that the two paths agree bit for bit, and one pa.generation.apply_augmentation with three ShiftAugments.
Reports ms for both, their ratio and the achieved GB/s against the compulsory bytes per voxel: 12 (field) + 4 + M read and
4 + M written = 36 for the fused call at M = 8, (1 + M) 12 + 2 (4 + M) = 132 for the member-by-member calls.
Prints one JSON line; --out writes it to a file."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import platipy_amd as pa  # noqa: E402
from platipy_amd import runtime  # noqa: E402


def phantom(size, nstruct, device):
    """A CT-like image (-1000 air, a soft ellipsoid body with noise) and ellipsoids of 0.1 % ... 5 % of the grid."""
    nx, ny, nz = size
    g = torch.Generator(device="cpu").manual_seed(11)
    z, y, x = torch.meshgrid(torch.arange(nz, device=device, dtype=torch.float32) / nz, torch.arange(ny, device=device, dtype=torch.float32) / ny,
                             torch.arange(nx, device=device, dtype=torch.float32) / nx, indexing="ij")
    body = (((x - 0.5) / 0.42) ** 2 + ((y - 0.5) / 0.4) ** 2 + ((z - 0.5) / 0.46) ** 2) < 1.0
    ct = torch.where(body, 40.0 * torch.sin(9.0 * x) * torch.cos(7.0 * y) + 30.0 * z, torch.full_like(x, -1000.0))
    ct = (ct + 5.0 * torch.randn((nz, ny, nx), generator=g).to(device)).contiguous()
    masks = []
    for frac in np.geomspace(0.001, 0.05, nstruct):
        a = (3.0 * frac / (4.0 * math.pi)) ** (1.0 / 3.0)
        c = (0.25 + 0.5 * torch.rand(3, generator=g)).tolist()
        masks.append(((((x - c[0]) / a) ** 2 + ((y - c[1]) / a) ** 2 + ((z - c[2]) / a) ** 2) <= 1.0).to(torch.uint8).contiguous())
    return ct, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--structures", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "augment_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench needs a GPU"
    dev = torch.device("cuda", 0)
    spacing = (0.98, 0.98, 2.5)
    ct_t, mask_t = phantom(a_.size, a_.structures, dev)
    ct = pa.Image(ct_t, spacing)
    masks = [pa.Image(m, spacing) for m in mask_t]
    n, nl = ct_t.numel(), len(masks)
    ctx = runtime.context(dev)
    # one smoothed field: noise on a coarse lattice spread by the recursive Gaussian (sigma 12 mm), scaled to 8 mm at its largest
    field = torch.zeros((3,) + tuple(ct_t.shape), dtype=torch.float32, device=dev)
    field[:, ::16, ::32, ::32] = torch.randn((3,) + tuple(field[0, ::16, ::32, ::32].shape), generator=torch.Generator().manual_seed(3)).to(dev)
    ctx.recursive_gaussian_field(field, ct.geom(), [12.0, 12.0, 12.0])
    field *= 8.0 / float(field.abs().max())
    transform = pa.DisplacementFieldTransform(pa.Image(field, spacing, is_vector=True))
    default = int(ct_t.min())

    def fused():
        return pa.registration.apply_transform_to_set(ct, masks, transform=transform, default_value=default, interpolator=pa.sitkLinear)

    def members():
        img = pa.registration.apply_transform(ct, transform=transform, default_value=default, interpolator=pa.sitkLinear)
        return img, [pa.registration.apply_transform(m, transform=transform, default_value=0, interpolator=pa.sitkNearestNeighbor) for m in masks]

    shifts = [pa.generation.ShiftAugment(masks[-1 - k], v, 5) for k, v in enumerate([(5, -7, 10), (-4, 6, 3), (8, 2, -6)])]

    def augmentation():
        return pa.generation.apply_augmentation(ct, shifts, masks)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for _ in range(2):      # warm-up, and the values
        got, want = fused(), members()
    assert torch.equal(got[0].tensor, want[0].tensor), "the fused image differs from apply_transform's"
    assert all(torch.equal(a.tensor, b.tensor) for a, b in zip(got[1], want[1])), "a fused label differs from apply_transform's"
    outside = float((got[0].tensor == default).double().mean())
    moved = float((got[0].tensor != ct_t).double().mean())
    del got, want
    tf, tm = [], []
    for _ in range(a_.reps):
        tf.append(event_ms(fused)[0])
        tm.append(event_ms(members)[0])
    augmentation()
    ta = [event_ms(augmentation)[0] for _ in range(a_.reps)]
    bf, bm = 12 + 2 * (4 + nl), (1 + nl) * 12 + 2 * (4 + nl)
    mf, mm = statistics.median(tf), statistics.median(tm)
    result = {"size": a_.size, "spacing": spacing, "structures": nl, "reps": a_.reps, "bit_identical": True,
              "field_abs_max_mm": round(float(field.abs().max()), 2), "voxels_changed": round(moved, 4), "voxels_at_default": round(outside, 4),
              "fused_ms_median": round(mf, 3), "fused_ms_min": round(min(tf), 3), "fused_ms_spread": round(max(tf) - min(tf), 3),
              "members_ms_median": round(mm, 3), "members_ms_min": round(min(tm), 3), "members_ms_spread": round(max(tm) - min(tm), 3),
              "members_over_fused": round(mm / mf, 2), "bytes_per_voxel_compulsory": {"fused": bf, "members": bm},
              "fused_compulsory_GB_per_s": round(bf * n / (mf * 1e-3) / 1e9, 1), "members_compulsory_GB_per_s": round(bm * n / (mm * 1e-3) / 1e9, 1),
              "apply_augmentation_3_shifts_ms_median": round(statistics.median(ta), 3), "apply_augmentation_ms_spread": round(max(ta) - min(ta), 3)}
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
