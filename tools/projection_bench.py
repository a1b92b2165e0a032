#!/usr/bin/env python
"""Rotated projections at the size of a planning CT: a seeded 512 x 512 x 256 fp32 phantom, spacing (0.98, 0.98, 2.5), and 8
uint8 ellipsoid structures (the phantom of tools/augment_bench.py).

Times, with HIP events (warm-up first, the two paths alternating inside every repetition, medians of --reps),
  * a rotating maximum-intensity projection: 72 views about z projected along y (axis 1), linear interpolation, ONE
    pa.visualisation.project_set call (pp_project_set) -- alone and with the 8 structures (nearest neighbour) --
  * single views about an oblique axis projected along each axis with max, mean and median,
each against the same planes composed from what the library had before: pa.utils.rotate_image (pp_resample_f32 / _u8) per
angle and member, then a torch reduction (amax; sum in float64 / n; kthvalue n // 2 + 1, the upper median).  The two paths
are compared in the run that times them: max, median and the label planes bit for bit; mean, whose torch sum adds in another
order, to the rounding of that sum (the largest difference is reported).
Reports ms for both, their ratio, and GB/s of the compulsory bytes: per view 4 B per voxel of image and 1 B per voxel and label
read, one fp32 plane and one uint8 plane per label written.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import platipy_amd as pa  # noqa: E402
from augment_bench import phantom  # noqa: E402  (the same seeded phantom, not a copy)
from platipy_amd.utils.geometry import rotate_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--structures", type=int, default=8)
    ap.add_argument("--views", type=int, default=72)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "projection_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "projection_bench needs a GPU"
    dev = torch.device("cuda", 0)
    V = pa.visualisation
    spacing = (0.98, 0.98, 2.5)
    ct_t, mask_t = phantom(a_.size, a_.structures, dev)
    ct = pa.Image(ct_t, spacing)
    masks = [pa.Image(m, spacing) for m in mask_t]
    nvox, nl = ct_t.numel(), len(masks)
    nx, _, nz = a_.size
    centre = [s * (n - 1) / 2.0 for s, n in zip(spacing, a_.size)]
    default = -1000
    angles = [2.0 * math.pi * k / a_.views for k in range(a_.views)]
    near, lin = pa.sitkNearestNeighbor, pa.sitkLinear

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def composed_image(kind, axis, rax, angle):
        rot = rotate_image(ct, centre, rax, angle, lin, default).tensor
        dim, n = 2 - axis, a_.size[axis]
        if kind == "max":
            return rot.amax(dim=dim)
        if kind == "mean":
            return (rot.sum(dim=dim, dtype=torch.float64) / n).float()
        return rot.kthvalue(n // 2 + 1, dim=dim).values      # the upper median

    def composed_label(mask, axis, rax, angle):
        return rotate_image(mask, centre, rax, angle, near, 0).tensor.amax(dim=2 - axis)

    def measure(name, fused, composed, exact, planes_bytes, read_bytes):
        for _ in range(2):      # warm-up, and the values
            got, want = fused(), composed()
        gi, gl = got
        wi, wl = want
        # what was observed: torch.equal of the image planes and of every label plane, and the largest difference
        same_image = bool(torch.equal(gi, wi))
        diff = float((gi.double() - wi.double()).abs().max())
        same_labels = len(gl) == len(wl) and all(torch.equal(a, b) for a, b in zip(gl, wl))
        if exact:
            assert same_image, f"{name}: the fused image planes differ from the composition's"
        else:
            assert diff <= 2.0 ** -22 * float(wi.abs().max()), f"{name}: {diff}"
        assert same_labels, f"{name}: a fused label plane differs"
        del got, want, gi, gl, wi, wl
        tf, tc = [], []
        for _ in range(a_.reps):
            tf.append(event_ms(fused)[0])
            tc.append(event_ms(composed)[0])
        mf, mc = statistics.median(tf), statistics.median(tc)
        return {"fused_ms_median": round(mf, 3), "fused_ms_min": round(min(tf), 3), "fused_ms_spread": round(max(tf) - min(tf), 3),
                "composed_ms_median": round(mc, 3), "composed_ms_min": round(min(tc), 3), "composed_ms_spread": round(max(tc) - min(tc), 3),
                "composed_over_fused": round(mc / mf, 3), "asserted": "bit-identical" if exact else "within the rounding of torch's sum",
                "image_planes_bit_identical": same_image, "label_planes_bit_identical": bool(same_labels), "max_abs_difference": diff,
                "compulsory_bytes": int(read_bytes + planes_bytes),
                "fused_compulsory_GB_per_s": round((read_bytes + planes_bytes) / (mf * 1e-3) / 1e9, 1)}

    result = {"size": a_.size, "spacing": spacing, "structures": nl, "views": a_.views, "reps": a_.reps, "interpolation": "linear (labels nearest)"}
    zax = (0.0, 0.0, 1.0)
    plane = nz * nx
    result["mip_72_views_axis1"] = measure(
        "rotating MIP", lambda: V.project_set(ct, [], angles, "max", 1, zax, default, lin),
        lambda: (torch.stack([composed_image("max", 1, zax, a) for a in angles]), []), True, a_.views * plane * 4, a_.views * nvox * 4)
    result["mip_72_views_axis1_with_labels"] = measure(
        "rotating MIP with labels", lambda: V.project_set(ct, masks, angles, "max", 1, zax, default, lin, near),
        lambda: (torch.stack([composed_image("max", 1, zax, a) for a in angles]),
                 [torch.stack([composed_label(m, 1, zax, a) for a in angles]) for m in masks]), True,
        a_.views * plane * (4 + nl), a_.views * nvox * (4 + nl))
    oblique, angle = (1.0, 2.0, 3.0), 0.3
    for axis in range(3):
        pixels = nvox // a_.size[axis]
        for kind in ("max", "mean", "median"):
            result[f"single_view_axis{axis}_{kind}"] = measure(
                f"axis {axis} {kind}", lambda: V.project_set(ct, [], [angle], kind, axis, oblique, default, lin),
                lambda: (composed_image(kind, axis, oblique, angle)[None], []), kind != "mean", pixels * 4, nvox * 4)
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
