#!/usr/bin/env python
"""get_external_mask and its kernels at the size of a planning CT: a seeded head-and-shoulders phantom of 512 x 512 x 256
(an ellipsoid head on wider shoulders, air cavities, a couch bar, noise specks in the air).

Times, with HIP events (warm-up first, medians of 5),
  * pp_slice_convex_hull_u8 on the body mask, in ms and as GB/s of its compulsory 2 bytes per voxel (one read, one write).
    A per-slice convex hull image has no torch composition -- there is no hull, sort-by-angle or per-slice scan primitive to
    compose it from, and the reference's own route is a Python loop over scikit-image on the host -- so no comparison is
    invented; the result is checked instead: it contains the mask, every row of it is one interval, and a second call gives
    the same bytes;
  * the 26-connected labelling (pp_connected_components_conn_u8) next to the face-connected call on the same thresholded
    mask in the same run, interleaved;
  * the whole get_external_mask(ct, dilate=15) of the head-and-neck walkthrough, as wall time around a device synchronise.
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
from platipy_amd import runtime  # noqa: E402


def phantom(size, seed, dev):
    """[Z][Y][X] float32 HU, built on the device from index grids."""
    nx, ny, nz = size
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    z = torch.arange(nz, device=dev, dtype=torch.float32)[:, None, None]
    y = torch.arange(ny, device=dev, dtype=torch.float32)[None, :, None]
    x = torch.arange(nx, device=dev, dtype=torch.float32)[None, None, :]
    img = torch.full((nz, ny, nx), -1000.0, device=dev)
    head = ((x - nx / 2) / (0.18 * nx)) ** 2 + ((y - 0.45 * ny) / (0.22 * ny)) ** 2 + ((z - 0.70 * nz) / (0.28 * nz)) ** 2 < 1
    shoulders = (((x - nx / 2) / (0.42 * nx)) ** 2 + ((y - 0.50 * ny) / (0.20 * ny)) ** 2 < 1) & (z < 0.38 * nz)
    neck = (((x - nx / 2) / (0.11 * nx)) ** 2 + ((y - 0.48 * ny) / (0.12 * ny)) ** 2 < 1) & (z < 0.75 * nz)
    img[head | shoulders | neck] = 40.0
    airway = (((x - nx / 2) / (0.02 * nx)) ** 2 + ((y - 0.42 * ny) / (0.025 * ny)) ** 2 < 1) & (z < 0.72 * nz)
    sinus = ((x - 0.46 * nx) / (0.04 * nx)) ** 2 + ((y - 0.33 * ny) / (0.04 * ny)) ** 2 + ((z - 0.74 * nz) / (0.05 * nz)) ** 2 < 1
    img[airway | sinus] = -1000.0
    couch = (y >= 0.74 * ny) & (y < 0.76 * ny) & (x >= 0.08 * nx) & (x < 0.92 * nx)
    img[couch.expand(nz, ny, nx)] = 250.0
    img += 8.0 * torch.randn((nz, ny, nx), device=dev, generator=g)
    specks = torch.rand((nz, ny, nx), device=dev, generator=g) < 2e-4
    img[specks & (img < -500.0)] = 400.0
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--seed", type=int, default=20240611)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "external_mask_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "external_mask_bench needs a GPU"
    dev = torch.device("cuda", 0)
    ctx = runtime.context(dev)
    nx, ny, nz = a_.size
    ct = pa.Image(phantom(a_.size, a_.seed, dev), (0.98, 0.98, 2.5), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), False)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(t):
        return {"ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_spread": round(max(t) - min(t), 3)}

    result = {"size": a_.size, "seed": a_.seed, "reps": a_.reps}
    thresholded = ((ct.tensor >= -100) & (ct.tensor <= 2500)).to(torch.uint8).contiguous()
    body = pa.label.largest_component(ct.like(thresholded), fully_connected=True).tensor.contiguous()
    result["thresholded_voxels"], result["body_voxels"] = int(thresholded.sum()), int(body.sum())

    # ---- the hull kernel ----
    hull, again = torch.empty_like(body), torch.empty_like(body)
    for _ in range(2):
        ctx.slice_convex_hull(body, a_.size, hull)
    t = [event_ms(lambda: ctx.slice_convex_hull(body, a_.size, hull)) for _ in range(a_.reps)]
    ctx.slice_convex_hull(body, a_.size, again)
    assert torch.equal(hull, again), "two calls of the hull kernel differ"
    assert bool(((hull != 0) | (body == 0)).all()), "the hull does not contain the mask"
    rises = ((hull[:, :, 1:] != 0) & (hull[:, :, :-1] == 0)).sum(dim=2) + (hull[:, :, 0] != 0)
    assert int(rises.max()) <= 1, "a row of the hull is not one interval"
    result["hull"] = dict(stats(t), voxels=int(hull.sum()), GB_per_s=round(2.0 * hull.numel() / (statistics.median(t) * 1e-3) / 1e9, 1),
                          bytes_per_voxel=2, torch_equivalent=None)

    # ---- 26-connected next to face-connected labelling, interleaved ----
    lab = torch.empty(thresholded.shape, dtype=torch.int32, device=dev)
    counts, times = {}, {"face": [], "full": []}
    for _ in range(2):
        ctx.connected_components(thresholded, a_.size, lab, want_count=False)
        ctx.connected_components_conn(thresholded, a_.size, lab, fully_connected=True, want_count=False)
    for _ in range(a_.reps):
        times["face"].append(event_ms(lambda: ctx.connected_components(thresholded, a_.size, lab, want_count=False)))
        times["full"].append(event_ms(lambda: ctx.connected_components_conn(thresholded, a_.size, lab, fully_connected=True, want_count=False)))
    counts["face"] = ctx.connected_components(thresholded, a_.size, lab)
    counts["full"] = ctx.connected_components_conn(thresholded, a_.size, lab, fully_connected=True)
    assert counts["full"] <= counts["face"]
    result["labelling"] = {k: dict(stats(times[k]), components=counts[k]) for k in ("face", "full")}
    result["labelling"]["full_over_face"] = round(statistics.median(times["full"]) / statistics.median(times["face"]), 3)

    # ---- the whole function ----
    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = pa.generation.get_external_mask(ct, dilate=15)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, m

    for _ in range(2):
        whole()
    runs = [whole() for _ in range(a_.reps)]
    result["get_external_mask_dilate_15"] = dict(stats([r[0] for r in runs]), voxels=int(runs[-1][1].tensor.sum()), clock="wall, synchronised")
    out_line = json.dumps(result)
    print(out_line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(out_line + "\n")


if __name__ == "__main__":
    main()
