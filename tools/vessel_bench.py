#!/usr/bin/env python
"""The two vessel-splining kernels at the size of a planning CT: 512 x 512 x 256, spacing (0.98, 0.98, 2.5).

Times, with HIP events (warm-up first, medians of 5),
  * pp_slice_moments_u8 for 10 propagated vessel labels (thin tubes, 0 / 1) on both scan axes, against the same int64 tables
    composed from torch (`sum` over one in-slice axis of the int64 volume, then an index-weighted `sum` over the other).
    The tables must be EQUAL: that is the tool's correctness check.  GB/s counts the compulsory read of 1 byte per voxel
    and mask;
  * pp_tube_mask_u8 for a 2 mm and a 10 mm tube around a centreline of about 2 500 segments (a gentle helix through the
    volume), in ms and as GB/s of its 1 byte per voxel of compulsory writes.  The entry synchronises and uploads the segment
    list, so the figure is the whole call's.  A tube has no torch equivalent at this size -- the distance of 67 M voxels to
    2 500 segments is 1.7e11 point-segment tests, or a 1.3 TB intermediate if it were written as one broadcast -- so none is
    invented; the voxel count is checked against the tube's analytic volume instead (within 10 %).
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
import platipy_amd as pa  # noqa: E402,F401
from platipy_amd import runtime  # noqa: E402


def helix(size, spacing, nseg):
    """nseg + 1 points of a helix of 1.5 turns around the volume's z axis, a quarter of the in-plane extent wide."""
    ext = [size[k] * spacing[k] for k in range(3)]
    t = np.linspace(0.0, 1.0, nseg + 1)
    return np.stack([ext[0] * (0.5 + 0.25 * np.cos(3.0 * math.pi * t)), ext[1] * (0.5 + 0.25 * np.sin(3.0 * math.pi * t)),
                     ext[2] * (0.1 + 0.8 * t)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--masks", type=int, default=10)
    ap.add_argument("--segments", type=int, default=2500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "vessel_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "vessel_bench needs a GPU"
    dev = torch.device("cuda", 0)
    nx, ny, nz = a_.size
    spacing, origin = (0.98, 0.98, 2.5), (0.0, 0.0, 0.0)
    ctx = runtime.context(dev)
    line = helix(a_.size, spacing, a_.segments)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def median_ms(fn):
        for _ in range(2):
            fn()
        t = [event_ms(fn)[0] for _ in range(a_.reps)]
        return round(statistics.median(t), 3), round(min(t), 3), round(max(t) - min(t), 3)

    result = {"size": a_.size, "spacing": spacing, "masks": a_.masks, "segments": a_.segments, "reps": a_.reps}

    # ---- tubes (they also serve as the vessel labels of the moments) ----
    tube = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
    length = float(np.sqrt((np.diff(line, axis=0) ** 2).sum(axis=1)).sum())
    for radius in (2.0, 10.0):
        med, lo, spread = median_ms(lambda: ctx.tube_mask(line, a_.size, spacing, origin, radius, tube))
        voxels = int(tube.sum())
        analytic = math.pi * radius * radius * length / (spacing[0] * spacing[1] * spacing[2])
        assert abs(voxels - analytic) <= 0.1 * analytic, (voxels, analytic)
        result[f"tube_{radius:g}mm"] = {"ms_median": med, "ms_min": lo, "ms_spread": spread, "voxels": voxels, "analytic_voxels": round(analytic),
                                        "write_GB_per_s": round(tube.numel() / (med * 1e-3) / 1e9, 1), "torch_equivalent": None}

    masks = []
    for k in range(a_.masks):       # the 2 mm tube, shifted a little per atlas
        ctx.tube_mask(line + np.array([1.3 * k, -0.9 * k, 0.0]), a_.size, spacing, origin, 2.0, tube)
        masks.append(tube.clone())
    stack = torch.stack(masks)
    iz = torch.arange(nz, device=dev, dtype=torch.int64)
    iy = torch.arange(ny, device=dev, dtype=torch.int64)
    ix = torch.arange(nx, device=dev, dtype=torch.int64)

    def composed(scan):
        out = []
        for m in masks:
            v = m.to(torch.int64)
            if scan == "z":
                rows = v.sum(dim=2)                      # [z, y]
                cols = v.sum(dim=1)                      # [z, x]
                out.append(torch.stack([rows.sum(dim=1), (rows * iy[None, :]).sum(dim=1), (cols * ix[None, :]).sum(dim=1),
                                        (m != 0).sum(dim=(1, 2))], dim=1))
            else:
                zx = v.sum(dim=1)                        # [z, x]
                yx = v.sum(dim=0)                        # [y, x]
                out.append(torch.stack([zx.sum(dim=0), (zx * iz[:, None]).sum(dim=0), (yx * iy[:, None]).sum(dim=0),
                                        (m != 0).sum(dim=(0, 1))], dim=1))
        return torch.stack(out)

    for scan, axis in (("z", 2), ("x", 0)):
        table = torch.empty((a_.masks, a_.size[axis], 4), dtype=torch.int64, device=dev)

        def kernel():
            ctx.slice_moments(masks, a_.size, axis, table)
            return table

        assert torch.equal(kernel(), composed(scan)), f"the composed {scan}-scan table differs from the kernel's"
        med, lo, spread = median_ms(kernel)
        cmed, clo, cspread = median_ms(lambda: composed(scan))
        result[f"moments_{scan}"] = {"new_ms_median": med, "new_ms_min": lo, "new_ms_spread": spread, "composed_ms_median": cmed,
                                     "composed_ms_min": clo, "composed_ms_spread": cspread, "composed_over_new": round(cmed / med, 2),
                                     "tables_equal": True, "read_GB_per_s": round(stack.numel() / (med * 1e-3) / 1e9, 1)}
    out_line = json.dumps(result)
    print(out_line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(out_line + "\n")


if __name__ == "__main__":
    main()
