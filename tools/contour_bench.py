#!/usr/bin/env python
"""RTSTRUCT contours to masks at the size of a planning CT: 512 x 512 x 256, 24 structures.

The input is a seeded phantom: every structure is an ellipsoid, every third one a ring (an inner contour on each slice, which
XOR turns into a hole), cut into per-slice polygons of about 200 integer vertices.

Times, with HIP events (warm-up first, medians of 5),
  * the whole pp_contour_fill_u8 call: host grouping, upload, zero fill, fill kernel, synchronisation;
  * its fill kernel alone and its zero fill alone (the library's own event brackets, Context.profile_enable);
  * pa.dicom.rasterise_contours on the same contours given as physical points (adds the fp64 transform on the host);
  * the same masks COMPOSED from torch: for every (structure, slice) a chunked [pixels x edges] int64 broadcast of the same
    integer rule over the job's clipped bounding box, XORed into a zeroed volume.  The two results must be EQUAL: that is
    the tool's correctness check.
GB/s counts the compulsory write of 1 byte per voxel and structure.  Prints one JSON line; --out writes it to a file."""
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
from platipy_amd import _lib, runtime  # noqa: E402


def phantom(size, nstructures, nverts, seed):
    """-> (vertices int64 [n, 2], contour table, jobs): jobs = [(structure, z, [(first, count), ...])]."""
    nx, ny, nz = size
    rng = np.random.default_rng(seed)
    t = 2.0 * math.pi * np.arange(nverts) / nverts
    verts, rows, jobs = [], [], []
    first = 0
    for s in range(nstructures):
        rx, ry, rz = rng.uniform(0.05, 0.2) * nx, rng.uniform(0.05, 0.2) * ny, rng.uniform(0.1, 0.4) * nz
        cx, cy, cz = rng.uniform(rx, nx - rx), rng.uniform(ry, ny - ry), rng.uniform(0.3, 0.7) * nz
        wobble = 1.0 + 0.08 * np.sin(rng.integers(2, 7) * t + rng.uniform(0, 6.0))
        ring = s % 3 == 2
        for z in range(max(0, int(math.ceil(cz - rz))), min(nz, int(cz + rz) + 1)):
            scale = math.sqrt(max(0.0, 1.0 - ((z - cz) / rz) ** 2))
            if scale * min(rx, ry) < 1.5:
                continue
            spans = []
            for k in ((1.0, 0.55) if ring else (1.0,)):
                x = np.floor(cx + k * scale * rx * wobble * np.cos(t) + 0.5).astype(np.int64)
                y = np.floor(cy + k * scale * ry * wobble * np.sin(t) + 0.5).astype(np.int64)
                verts.append(np.stack([x, y], axis=1))
                rows.append((first, nverts, s, z))
                spans.append((first, nverts))
                first += nverts
            jobs.append((s, z, spans))
    return np.concatenate(verts), np.array(rows, dtype=_lib.CONTOUR_DTYPE), jobs


def composed(dverts, jobs, size, nstructures, budget=1 << 24):
    """The same masks from torch int64 broadcasts: the rule of csrc/pp_contour.h, pixels x edges, chunked over pixels."""
    nx, ny, nz = size
    dev = dverts.device
    out = torch.zeros((nstructures, nz, ny, nx), dtype=torch.uint8, device=dev)
    for s, z, spans in jobs:
        lo = torch.stack([dverts[f:f + c].min(dim=0).values for f, c in spans]).min(dim=0).values.tolist()
        hi = torch.stack([dverts[f:f + c].max(dim=0).values for f, c in spans]).max(dim=0).values.tolist()
        x0, x1, y0, y1 = max(lo[0], 0), min(hi[0], nx - 1), max(lo[1], 0), min(hi[1], ny - 1)
        if x1 < x0 or y1 < y0:
            continue
        w = x1 - x0 + 1
        py, px = torch.meshgrid(torch.arange(y0, y1 + 1, device=dev), torch.arange(x0, x1 + 1, device=dev), indexing="ij")
        px, py = px.reshape(-1, 1), py.reshape(-1, 1)
        value = torch.zeros(px.shape[0], dtype=torch.bool, device=dev)
        for f, c in spans:
            b = dverts[f:f + c]
            a = torch.roll(b, 1, dims=0)
            ax, ay, bx, by = a[:, 0][None], a[:, 1][None], b[:, 0][None], b[:, 1][None]
            cross, dya, den = ax * by - ay * bx, ay - by, ax - bx
            step = max(1, budget // c)
            for p0 in range(0, px.shape[0], step):
                qx, qy = px[p0:p0 + step], py[p0:p0 + step]
                num = cross + qx * dya - qy * den
                sign = torch.sign(num) * torch.sign(den)
                v0, v1 = ax - qx, bx - qx
                right = (((v1 > 0) != (v0 > 0)) & (sign > 0)).sum(dim=1)
                left = (((v1 < 0) != (v0 < 0)) & (sign < 0)).sum(dim=1)
                vertex = ((v1 == 0) & (by == qy)).any(dim=1)
                value[p0:p0 + step] ^= vertex | (right % 2 == 1) | (left % 2 == 1)
        out[s, z, y0:y1 + 1, x0:x1 + 1] = value.reshape(-1, w).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--structures", type=int, default=24)
    ap.add_argument("--vertices", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20240611)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "contour_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "contour_bench needs a GPU"
    dev = torch.device("cuda", 0)
    nx, ny, nz = a_.size
    S = a_.structures
    ctx = runtime.context(dev)
    verts, table, jobs = phantom(a_.size, S, a_.vertices, a_.seed)
    out = torch.empty((S, nz, ny, nx), dtype=torch.uint8, device=dev)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def median_ms(fn, warm=2):
        for _ in range(warm):
            fn()
        t = [event_ms(fn)[0] for _ in range(a_.reps)]
        return round(statistics.median(t), 3), round(min(t), 3), round(max(t) - min(t), 3)

    result = {"size": a_.size, "structures": S, "vertices_per_contour": a_.vertices, "contours": int(table.size), "jobs": len(jobs),
              "vertices": int(verts.shape[0]), "reps": a_.reps, "seed": a_.seed}
    nbytes = out.numel()

    def call():
        ctx.contour_fill(verts, table, a_.size, S, out)

    med, lo, spread = median_ms(call)
    result["call"] = {"ms_median": med, "ms_min": lo, "ms_spread": spread, "write_GB_per_s": round(nbytes / (med * 1e-3) / 1e9, 1)}
    result["inside_voxels"] = int(out.sum(dtype=torch.int64))

    # the call's two device steps, by the library's own event brackets
    ctx.profile_enable(True)
    ctx.profile_read()
    parts = {"k_contour_fill": [], "contour_zero_fill": []}
    for _ in range(a_.reps):
        call()
        prof = ctx.profile_read()
        for name in parts:
            parts[name].append(prof[name][1])
    ctx.profile_enable(False)
    for name, key in (("k_contour_fill", "fill_kernel"), ("contour_zero_fill", "zero_fill")):
        m = statistics.median(parts[name])
        result[key] = {"ms_median": round(m, 3), "ms_min": round(min(parts[name]), 3), "ms_spread": round(max(parts[name]) - min(parts[name]), 3),
                       "write_GB_per_s": round(nbytes / (m * 1e-3) / 1e9, 1) if key == "zero_fill" else None}
    result["device_steps_write_GB_per_s"] = round(nbytes / ((result["fill_kernel"]["ms_median"] + result["zero_fill"]["ms_median"]) * 1e-3) / 1e9, 1)

    # the public entry on physical points
    spacing, origin = (0.98, 0.98, 2.5), (-250.0, -250.0, 40.0)
    ref = pa.Image(torch.zeros((nz, ny, nx), dtype=torch.int16, device=dev), spacing, origin)
    per_structure = {f"s{s}": [] for s in range(S)}
    for first, count, s, z in table.tolist():
        idx = np.concatenate([verts[first:first + count], np.full((count, 1), z)], axis=1).astype(np.float64)
        per_structure[f"s{s}"].append(np.asarray(origin) + idx * np.asarray(spacing))
    stack, _ = pa.dicom.rasterise_contours(ref, per_structure, as_dict=False)
    result["rasterise_contours_equal"] = bool(torch.equal(stack, out))
    med, lo, spread = median_ms(lambda: pa.dicom.rasterise_contours(ref, per_structure, as_dict=False), warm=1)
    result["rasterise_contours"] = {"ms_median": med, "ms_min": lo, "ms_spread": spread}
    del stack

    # the same masks composed from torch
    dverts = torch.from_numpy(verts).to(dev)
    want = composed(dverts, jobs, a_.size, S)
    result["equal"] = bool(torch.equal(want, out))
    del want
    cmed, clo, cspread = median_ms(lambda: composed(dverts, jobs, a_.size, S), warm=0)
    result["composed"] = {"ms_median": cmed, "ms_min": clo, "ms_spread": cspread}
    result["composed_over_call"] = round(cmed / result["call"]["ms_median"], 1)
    assert result["equal"] and result["rasterise_contours_equal"], "the composed masks differ from the kernel's"
    out_line = json.dumps(result)
    print(out_line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(out_line + "\n")


if __name__ == "__main__":
    main()
