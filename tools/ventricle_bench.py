#!/usr/bin/env python
"""The left-ventricle 17-segment model at the size of a cropped heart: 160 x 160 x 120 voxels of 1 mm.

Times, with HIP events (warm-up first, medians of 5),
  * pp_polar_sectors_u8 on a myocardium shell standing along z (apex segment, apical quarters, mid and basal sixths, the
    slice centres truncated centres of mass) against the same 17 masks composed from torch in fp64: atan2, the single + 2 pi,
    sqrt, the comparisons of every sector, per-slice sums and the area test.  The two results must be EQUAL: that is the
    tool's correctness check (both sides call the device library's atan2).  The entry uploads its tables and synchronises, so
    the figure is the whole call's;
  * pp_resample_bits_u32 of that bit image through an oblique rigid transform against 17 apply_transform calls (nearest
    neighbour) on the 17 uint8 masks.  Every plane must be EQUAL;
  * generate_left_ventricle_segments on a phantom of tilted ellipsoid chambers (the one of tests/test_ventricle.py, scaled
    by 1.1), wall clock around a synchronise -- the function reads scalars back between its stages.
Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import platipy_amd as pa  # noqa: E402
from platipy_amd import _lib, runtime  # noqa: E402
from platipy_amd.utils import ventricle as VT  # noqa: E402


def heart_phantom(shape, spacing, scale):
    """Tilted ellipsoid chambers ([Z][Y][X] uint8): the long axis leans 25 degrees away from -z."""
    sp = np.asarray(spacing, dtype=np.float64)
    z, y, x = np.indices(shape).astype(np.float64)
    p = np.stack([x * sp[0], y * sp[1], z * sp[2]], axis=-1)
    c = 0.5 * np.asarray(shape[::-1], dtype=np.float64) * sp
    s25, c25 = np.sin(np.radians(25.0)), np.cos(np.radians(25.0))
    l = np.array([0.8 * s25, 0.6 * s25, -c25])
    l /= np.linalg.norm(l)
    u = np.cross(l, (0.0, 1.0, 0.0))
    u /= np.linalg.norm(u)
    v = np.cross(l, u)
    lv_c = c + 4.0 * scale * l

    def ellipsoid(centre, semi):
        d = p - centre
        return ((d @ u) / (semi[0] * scale)) ** 2 + ((d @ v) / (semi[1] * scale)) ** 2 + ((d @ l) / (semi[2] * scale)) ** 2 <= 1

    along = (p - lv_c) @ l
    heart = (((p - c) / (np.array([44.0, 44.0, 54.0]) * scale)) ** 2).sum(axis=-1) <= 1
    lv = ellipsoid(lv_c, (24, 24, 38)) & (along >= -14 * scale)
    la = ellipsoid(lv_c - 25 * scale * l, (16, 16, 11)) & (along < -14 * scale)
    rv = ellipsoid(lv_c + 24 * scale * u + 2 * scale * l, (16, 24, 40)) & ~lv & ~la & (along >= -14 * scale)
    return {"Ventricle_L": lv.astype(np.uint8), "Atrium_L": la.astype(np.uint8), "Ventricle_R": rv.astype(np.uint8), "Heart": heart.astype(np.uint8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[160, 160, 120], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "ventricle_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "ventricle_bench needs a GPU"
    dev = torch.device("cuda", 0)
    nx, ny, nz = a_.size
    shape = (nz, ny, nx)
    ctx = runtime.context(dev)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median_ms(fn):
        for _ in range(2):
            fn()
        t = [event_ms(fn) for _ in range(a_.reps)]
        return round(statistics.median(t), 3), round(min(t), 3), round(max(t) - min(t), 3)

    result = {"size": a_.size, "spacing": (1.0, 1.0, 1.0), "reps": a_.reps}

    # ---- the myocardium shell, standing along z, and its tables ----
    z, y, x = np.indices(shape).astype(np.float64)
    cz, cy, cx = 0.45 * nz, 0.5 * ny + 0.3, 0.5 * nx - 0.4

    def ell(a, b, c):
        return ((x - cx) / a) ** 2 + ((y - cy) / b) ** 2 + ((z - cz) / c) ** 2 <= 1

    myo = (ell(26.4, 26.4, 41.8) & ~ell(16.4, 16.4, 31.8) & (z <= cz + 15)).astype(np.uint8)
    inf_limit = int(np.ceil(cz - 31.8))
    basal = int(cz + 15) + 1
    dc = (basal - inf_limit) // 3
    apical, mid = inf_limit + dc, inf_limit + 2 * dc
    theta_0, theta_0_apical = 0.35, -0.17
    rules = [(lab, _lib.POLAR_CW if cw else 0, a0, a1) for lab, cw, a0, a1 in VT.APICAL_RULES + VT.MID_RULES + VT.BASAL_RULES]
    rules.append((17, _lib.POLAR_ANY_AREA, -np.inf, np.inf))
    slices = []
    for k in range(nz):
        if k < inf_limit:
            slices.append((0.0, 0.0, 0.0, 0.0, 16, 1))
        elif k >= basal or not myo[k].any():
            slices.append((0.0, 0.0, 0.0, 0.0, 0, 0))
        else:
            yy, xx = np.nonzero(myo[k])
            y0, x0 = float(int(yy.mean())), float(int(xx.mean()))
            slices.append((y0, x0, theta_0_apical, 0.0, 0, 4) if k < apical else
                          ((y0, x0, theta_0, 0.0, 4, 6) if k < mid else (y0, x0, theta_0, 15.0, 10, 6)))
    st = np.array(slices, dtype=_lib.POLAR_SLICE_DTYPE)
    rt = np.array(rules, dtype=_lib.POLAR_RULE_DTYPE)
    area, min_area = 1.0, 50.0
    dmyo = torch.from_numpy(myo).to(dev)
    bits = torch.empty(shape, dtype=torch.int32, device=dev)
    counts = torch.empty((nz, 32), dtype=torch.int64, device=dev)

    def kernel():
        ctx.polar_sectors(dmyo, a_.size, st, rt, area, min_area, bits, counts)

    # the same from torch: per-slice parameters as [Z, 1, 1] tensors, one mask per segment
    t_cy = torch.tensor(st["cy"], device=dev).view(nz, 1, 1)
    t_cx = torch.tensor(st["cx"], device=dev).view(nz, 1, 1)
    t_t0 = torch.tensor(st["theta0"], device=dev).view(nz, 1, 1)
    t_rmin = torch.tensor(st["radius_min"], device=dev).view(nz, 1, 1)
    gy = torch.arange(ny, device=dev, dtype=torch.float64).view(1, ny, 1)
    gx = torch.arange(nx, device=dev, dtype=torch.float64).view(1, 1, nx)
    uses = torch.zeros((nz, len(rules)), dtype=torch.bool)
    for k, s in enumerate(slices):
        uses[k, s[4]:s[4] + s[5]] = True
    uses = uses.to(dev)

    def composed():
        dy, dx = gy - t_cy, gx - t_cx
        theta = -torch.atan2(dy, dx) - t_t0
        theta = torch.where(theta < 0, theta + 2 * np.pi, theta)
        r = torch.sqrt(dy * dy + dx * dx)
        inside = (dmyo != 0) & (r >= t_rmin)
        out = []
        for k, (lab, flags, a0, a1) in enumerate(rules):
            m = ((theta <= a0) | (theta >= a1)) if flags & _lib.POLAR_CW else ((theta >= a0) & (theta <= a1))
            m = m & inside & uses[:, k].view(nz, 1, 1)
            if not flags & _lib.POLAR_ANY_AREA:
                m = m & ~(m.sum(dim=(1, 2), keepdim=True).to(torch.float64) * area < min_area)
            out.append((lab, m.to(torch.uint8)))
        return out

    kernel()
    masks = [torch.zeros(shape, dtype=torch.uint8, device=dev) for _ in range(17)]
    for lab, m in composed():
        masks[lab - 1] |= m
    for k in range(17):
        assert torch.equal(((bits >> k) & 1).to(torch.uint8), masks[k]), f"segment {k + 1}: the composed mask differs from the kernel's"
    med, lo, spread = median_ms(kernel)
    cmed, clo, cspread = median_ms(composed)
    result["polar_sectors"] = {"new_ms_median": med, "new_ms_min": lo, "new_ms_spread": spread, "composed_ms_median": cmed, "composed_ms_min": clo,
                               "composed_ms_spread": cspread, "composed_over_new": round(cmed / med, 2), "masks_equal": True,
                               "mask_voxels": int(myo.sum()), "rules_per_call": len(rules)}

    # ---- the way back: one gather against seventeen ----
    geom = _lib.make_geom(a_.size)
    t = pa.transform.VersorRigid3DTransform()
    t.SetCenter((0.5 * nx + 0.25, 0.5 * ny - 0.4, 0.5 * nz + 0.1))
    t.SetRotation((1.0, 2.0, 3.0), 0.5)
    A, off = t.matrix_offset()
    planes = torch.empty((17,) + shape, dtype=torch.uint8, device=dev)
    images = [pa.Image(m) for m in masks]

    def fused():
        ctx.resample_bits(bits, geom, geom, 17, planes, affine_A=A.ravel(), affine_t=off)

    def seventeen():
        return [pa.registration.utils.apply_transform(im, im, t, 0, pa.transform.sitkNearestNeighbor) for im in images]

    fused()
    for k, im in enumerate(seventeen()):
        assert torch.equal(planes[k], im.tensor), f"plane {k}: the fused gather differs from apply_transform"
    med, lo, spread = median_ms(fused)
    cmed, clo, cspread = median_ms(seventeen)
    result["resample_bits"] = {"new_ms_median": med, "new_ms_min": lo, "new_ms_spread": spread, "composed_ms_median": cmed, "composed_ms_min": clo,
                               "composed_ms_spread": cspread, "composed_over_new": round(cmed / med, 2), "planes_equal": True}

    # ---- the whole function ----
    arrays = heart_phantom(shape, (1.0, 1.0, 1.0), 1.1)
    contours = {k: pa.image_from_array(v, (1.0, 1.0, 1.0)) for k, v in arrays.items()}
    info = {}
    out = pa.utils.generate_left_ventricle_segments(contours, info=info)
    times = []
    for _ in range(a_.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pa.utils.generate_left_ventricle_segments(contours)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    result["whole_function"] = {"wall_ms_median": round(statistics.median(times), 2), "wall_ms_min": round(min(times), 2),
                                "wall_ms_spread": round(max(times) - min(times), 2), "rotations": len(info["rotation_angles"]),
                                "segment_voxels": [int(v.tensor.sum()) for v in out.values()]}
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
