#!/usr/bin/env python
"""Airway and lung segmentation at the size of a thoracic CT: the thorax phantom of tests/bronchus_restatement.py scaled to
512 x 512 x 160 voxels at 1 mm (built on the device).

Times, with HIP events (warm-up first, medians of --reps, the two paths alternating inside every repetition), each region
kernel of csrc/pp_region.h against the same result COMPOSED from what existed before it:
  * numbering   pp_connected_components_u8 (labelling + ranking of the roots) against the existing labelling entry point
                (pp_fillhole_largest_component_u8 without hole filling: label, count, arg max, select) followed by
                torch.unique(return_inverse=True) on the compressed roots
  * moments     pp_label_moments_i32 against ten torch.bincount calls with weights (index grids built outside the timing;
                bincount sums in fp64, exact here because every sum is below 2^53)
  * region grow pp_connected_threshold_f32 against threshold + labelling + compare with the seed's label
  * median      pp_binary_median_u8 against avg_pool3d over the replicate-padded mask
and the whole run_bronchus_segmentation (host clock around a synchronise), with the share of it spent in the region grows.
The composed results must EQUAL the kernels': that is the tool's correctness check.  The size range of the airway search is
scaled with the phantom's physical volume.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import platipy_amd as pa  # noqa: E402
from platipy_amd import runtime  # noqa: E402


def capsule(zz, yy, xx, a, b, radius):
    az, ay, ax = a
    dz, dy, dx = b[0] - az, b[1] - ay, b[2] - ax
    t = (((zz - az) * dz + (yy - ay) * dy + (xx - ax) * dx) / (dz * dz + dy * dy + dx * dx)).clamp_(0.0, 1.0)
    return (zz - (az + t * dz)) ** 2 + (yy - (ay + t * dy)) ** 2 + (xx - (ax + t * dx)) ** 2 <= radius * radius


def phantom(size, device):
    """The test phantom's shapes in ITS voxel units (96 x 96 x 80), sampled on a grid of `size`."""
    nx, ny, nz = size
    z = (torch.arange(nz, device=device, dtype=torch.float32) * (80.0 / nz)).view(-1, 1, 1)
    y = (torch.arange(ny, device=device, dtype=torch.float32) * (96.0 / ny)).view(1, -1, 1)
    x = (torch.arange(nx, device=device, dtype=torch.float32) * (96.0 / nx)).view(1, 1, -1)
    zz, yy, xx = torch.broadcast_tensors(z, y, x)
    img = torch.full((nz, ny, nx), -1000.0, device=device)
    img[((xx - 47.5) / 40) ** 2 + ((yy - 47.5) / 30) ** 2 <= 1] = 0.0
    for sx in (-18, 18):
        img[((zz - 30) / 20) ** 2 + ((yy - 48) / 16) ** 2 + ((xx - (48 + sx)) / 12) ** 2 <= 1] = -800.0
    img[capsule(zz, yy, xx, (42, 48, 48), (85, 48, 48), 3.6)] = -870.0
    img[capsule(zz, yy, xx, (42, 48, 48), (85, 48, 48), 2.5)] = -1000.0
    for sx in (-16, 16):
        img[capsule(zz, yy, xx, (42, 48, 48), (32, 48, 48 + sx), 1.6)] = -1000.0
    img[(zz >= 70) & (zz < 72) & (yy >= 30) & (yy < 32) & (xx >= 30) & (xx < 32)] = -1000.0
    return img.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 160], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "bronchus_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "bronchus_bench needs a GPU"
    dev = torch.device("cuda", 0)
    nx, ny, nz = a_.size
    size, n = (nx, ny, nz), nx * ny * nz
    spacing = (1.0, 1.0, 1.0)
    ct_t = phantom(size, dev)
    ct = pa.Image(ct_t, spacing)
    ctx = runtime.context(dev)
    volume_scale = (96.0 / nx) * (96.0 / ny) * (80.0 / nz) * 27.0          # test phantom mm^3 per bench phantom mm^3
    settings = dict(pa.projects.BRONCHUS_SETTINGS_DEFAULTS)
    settings["algorithmSettings"] = dict(pa.projects.bronchus.default_settings,
                                         expected_physical_size_range=[round(22000 / volume_scale), round(150000 / volume_scale)],
                                         minimum_tree_half_physical_size=round(1000 / volume_scale))

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    air = ((ct_t >= -10000) & (ct_t <= -400)).to(torch.uint8).contiguous()
    labels = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
    count = ctx.connected_components(air, size, labels)
    flat = labels.reshape(-1).long()
    lin = torch.arange(n, device=dev)
    first = torch.full((count + 1,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, flat, lin, reduce="amin")
    roots = torch.where(flat > 0, first[flat], torch.full_like(flat, -1)).to(torch.int32)       # what k_cc_compress leaves, background -1
    scratch_u8 = torch.empty_like(air)

    def numbering_new():
        out = torch.empty_like(labels)
        return out, ctx.connected_components(air, size, out)

    def numbering_old():
        ctx.fillhole_largest_component(air, size, scratch_u8, fill_holes=False)
        u, inv = torch.unique(roots, return_inverse=True)
        return inv.to(torch.int32).reshape(nz, ny, nx), int(u.numel()) - 1

    zi, yi, xi = [g.reshape(-1).double() for g in torch.meshgrid(torch.arange(nz, device=dev), torch.arange(ny, device=dev),
                                                                  torch.arange(nx, device=dev), indexing="ij")]
    weights = [None, xi, yi, zi, xi * xi, yi * yi, zi * zi, xi * yi, xi * zi, yi * zi]

    def moments_new():
        out = torch.empty((count, 10), dtype=torch.int64, device=dev)
        ctx.label_moments(labels, size, count, out)
        return out

    def moments_old():
        cols = [torch.bincount(flat, weights=w, minlength=count + 1)[1:] for w in weights]
        return torch.stack([c.round().long() if c.is_floating_point() else c for c in cols], dim=1)

    seed = [int(round(48 * nx / 96.0)), int(round(48 * ny / 96.0)), int(round(72 * nz / 80.0))]
    hu = -900.0

    def grow_new():
        out = torch.empty_like(air)
        ctx.connected_threshold(ct_t, size, -2000.0, hu, [seed], out)
        return out

    def grow_old():
        m = ((ct_t >= -2000.0) & (ct_t <= hu)).to(torch.uint8)
        lab = torch.empty_like(labels)
        ctx.connected_components(m, size, lab, want_count=False)
        s = lab[seed[2], seed[1], seed[0]]
        return ((lab == s) & (lab > 0)).to(torch.uint8)

    def median_new():
        out = torch.empty_like(air)
        ctx.binary_median(air, size, (1, 1, 1), out)
        return out

    def median_old():
        p = F.pad(air.float()[None, None], (1, 1, 1, 1, 1, 1), mode="replicate")
        return (F.avg_pool3d(p, 3, stride=1)[0, 0] > 0.5).to(torch.uint8)

    cases = {"numbering": (numbering_new, numbering_old), "moments": (moments_new, moments_old), "region_grow": (grow_new, grow_old),
             "median": (median_new, median_old)}
    result = {"size": list(size), "spacing": spacing, "reps": a_.reps, "components": count, "seed": seed, "hu": hu}
    for name, (new, old) in cases.items():
        for _ in range(2):
            vn, vo = new(), old()
        if name == "numbering":
            assert vn[1] == vo[1] == count and torch.equal(vn[0], vo[0]), "the composed numbering differs from the kernel's"
        else:
            assert torch.equal(vn, vo), f"{name}: the composed result differs from the kernel's"
        del vn, vo
        tn, to = [], []
        for _ in range(a_.reps):
            tn.append(event_ms(new)[0])
            to.append(event_ms(old)[0])
        result[name] = {"new_ms_median": round(statistics.median(tn), 3), "new_ms_min": round(min(tn), 3), "new_ms_max": round(max(tn), 3),
                        "composed_ms_median": round(statistics.median(to), 3), "composed_ms_min": round(min(to), 3),
                        "composed_ms_max": round(max(to), 3), "composed_over_new": round(statistics.median(to) / statistics.median(tn), 2),
                        "equal": True}
    result["moments"]["GB_per_s"] = round(4.0 * n / (result["moments"]["new_ms_median"] * 1e-3) / 1e9, 1)

    def pipeline():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pa.projects.run_bronchus_segmentation(ct, settings)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    pipeline()
    times = []
    for _ in range(a_.reps):
        ms, res = pipeline()
        times.append(ms)
    info = pa.projects.bronchus.run_bronchus_segmentation.last_info
    grows = len(info["candidates"])
    total = statistics.median(times)
    result["pipeline"] = {"ms_median": round(total, 2), "ms_min": round(min(times), 2), "ms_max": round(max(times), 2),
                          "structures": sorted(res), "lung_voxels": int(res[settings["outputLungName"]].tensor.sum(dtype=torch.int64)),
                          "bronchus_voxels": int(res[settings["outputBronchusName"]].tensor.sum(dtype=torch.int64)) if settings["outputBronchusName"] in res else None,
                          "seed": info["seed"], "lung_mask_hu": info["lung_mask_hu"], "distance_from_sup_slice": info["distance_from_sup_slice"],
                          "carina_slice": info["carina_slice"], "region_grows": grows,
                          "region_grow_share": round(grows * result["region_grow"]["new_ms_median"] / total, 3),
                          "size_range": settings["algorithmSettings"]["expected_physical_size_range"]}
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
