#!/usr/bin/env python
"""Label comparison metrics (platipy_amd.label.comparison) at the size of a planning CT: 512 x 512 x 256 voxels, two shifted
ellipsoids, spacing (0.9, 1.1, 2.5).

Times compute_surface_metrics, compute_volume_metrics and compute_metric_total_apl with HIP events (warm-up first, the
two paths alternating inside every repetition) against the same quantities COMPOSED from what the package exported before
this module existed -- label.distance_map, label.label_contour, label.binary_dilate, boolean indexing and torch
reductions, the way evaluate_distance_to_reference works -- and checks that both give the same numbers.  Also times the four
distance maps one compute_surface_metrics call needs, to report their share.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import platipy_amd as pa  # noqa: E402
from platipy_amd.label import comparison as C  # noqa: E402


def ellipsoid_pair(size, device):
    nx, ny, nz = size
    z, y, x = torch.meshgrid(torch.arange(nz, device=device, dtype=torch.float32), torch.arange(ny, device=device, dtype=torch.float32),
                             torch.arange(nx, device=device, dtype=torch.float32), indexing="ij")

    def one(c, r):
        return ((((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2) <= 1.0).to(torch.uint8)

    r = (0.14 * nx, 0.12 * ny, 0.12 * nz)
    return one((0.50 * nx, 0.50 * ny, 0.50 * nz), r), one((0.50 * nx - 4, 0.50 * ny + 5, 0.50 * nz + 3), r)


def border26(mask):
    """BinaryContour(fullyConnected) with torch: object voxels whose 3x3x3 neighbourhood (inside the image) holds background."""
    bg = (mask == 0).to(torch.float32)[None, None]
    return (mask != 0) & (F.max_pool3d(bg, 3, stride=1, padding=1)[0, 0] > 0)


def composed_surface_metrics(a, b):
    mean, mx, std, med, n, hd = [], [], [], [], [], []
    for la, lb in ((a, b), (b, a)):
        d = pa.label.distance_map(la, signed=True).tensor
        ad = d.abs()
        v = ad[pa.label.label_contour(lb).tensor == 1]
        lo, hi = ad.min(), ad.max()
        cum = torch.cumsum(torch.histc(v, 128, float(lo), float(hi)), 0)
        i = int(torch.searchsorted(cum, cum[-1:] / 2.0)[0])
        v64 = v.double()
        n.append(v.numel())
        mean.append(float(v64.mean()))
        std.append(float(v64.std()))
        mx.append(float(v.max()))
        med.append(float(lo) + (i + 0.5) * (float(hi) - float(lo)) / 128)
        hd.append(float(d[lb.tensor != 0].clamp(min=0).max()))
    ca, cb = border26(a.tensor), border26(b.tensor)
    da = pa.label.distance_map(a.like(ca.to(torch.uint8)), signed=True).tensor
    db = pa.label.distance_map(a.like(cb.to(torch.uint8)), signed=True).tensor
    near = int((cb & (da <= 3.0)).sum()) + int((ca & (db <= 3.0)).sum())
    mean_all = np.dot(mean, n) / np.sum(n)
    return {
        "hausdorffDistance": max(hd),
        "hausdorffDistance95": float(np.percentile(mx, 95)),
        "meanSurfaceDistance": float(mean_all),
        "medianSurfaceDistance": float(np.mean(med)),
        "maximumSurfaceDistance": float(np.max(mx)),
        "sigmaSurfaceDistance": float(np.sqrt(np.dot(n, np.add(np.square(std), np.square(np.subtract(mean, mean_all)))))),
        "surfaceDSC": near / (int(ca.sum()) + int(cb.sum())),
    }


def composed_volume_metrics(a, b):
    fa, fb = a.tensor != 0, b.tensor != 0
    na, nb, nab, n = int(fa.sum()), int(fb.sum()), int((fa & fb).sum()), fa.numel()
    return C._volume_metrics(na, nb, nab, n, a.GetSpacing())


def contour4(t):
    """2-D LabelContour of every slice with torch: object voxels with an in-plane face neighbour that is background."""
    f = (t != 0).to(torch.uint8)
    p = F.pad(f, (1, 1, 1, 1), value=1)
    return (f & (1 - (p[:, 1:-1, :-2] & p[:, 1:-1, 2:] & p[:, :-2, 1:-1] & p[:, 2:, 1:-1]))) != 0


def composed_total_apl(ref, test, threshold=3):
    r = int(np.ceil(threshold / np.mean(ref.GetSpacing()[:2])))
    rc, tc = contour4(ref.tensor), contour4(test.tensor)
    tc = pa.label.binary_dilate(ref.like(tc.to(torch.uint8)), [r, r, 0]).tensor != 0
    added = (rc & ~tc).sum(dim=(1, 2))
    keep = ((ref.tensor != 0).sum(dim=(1, 2)) + (test.tensor != 0).sum(dim=(1, 2))) != 0
    return float(added[keep].sum().cpu()) * float(np.mean(ref.GetSpacing()[:2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "comparison_bench needs a GPU"
    dev = torch.device("cuda", 0)
    ta, tb = ellipsoid_pair(a_.size, dev)
    spacing = (0.9, 1.1, 2.5)
    a, b = pa.Image(ta, spacing), pa.Image(tb, spacing)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def four_maps():
        for t in (ta, tb, ta, tb):      # two labels + two contour images: the map's cost does not depend on the content much
            pa.label.distance_map(a.like(t), signed=True)

    cases = {
        "surface_metrics": (lambda: C.compute_surface_metrics(a, b), lambda: composed_surface_metrics(a, b)),
        "volume_metrics": (lambda: C.compute_volume_metrics(a, b), lambda: composed_volume_metrics(a, b)),
        "total_apl": (lambda: C.compute_metric_total_apl(a, b), lambda: composed_total_apl(a, b)),
        "four_distance_maps": (four_maps, None),
    }
    result = {"size": a_.size, "spacing": spacing, "reps": a_.reps, "voxels_a": int(ta.sum()), "voxels_b": int(tb.sum())}
    for name, (new, old) in cases.items():
        vn, vo = new(), (old() if old else None)      # warm-up, and the values
        tn, to = [], []
        for _ in range(a_.reps):
            tn.append(event_ms(new)[0])
            if old:
                to.append(event_ms(old)[0])
        entry = {"new_ms_median": round(statistics.median(tn), 3), "new_ms_min": round(min(tn), 3),
                 "new_ms_spread": round(max(tn) - min(tn), 3)}
        if old:
            entry.update({"composed_ms_median": round(statistics.median(to), 3), "composed_ms_min": round(min(to), 3),
                          "composed_ms_spread": round(max(to) - min(to), 3), "new_value": vn, "composed_value": vo})
        result[name] = entry
    result["distance_map_share_of_surface_metrics"] = round(result["four_distance_maps"]["new_ms_median"] /
                                                            result["surface_metrics"]["new_ms_median"], 3)
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
