#!/usr/bin/env python
"""Dose-volume histograms at the size of a planning CT: a 512 x 512 x 256 dose, spacing (0.98, 0.98, 2.5), and 8 ellipsoid
structures that cover 0.1 % ... 5 % of the volume each.

Times, with HIP events (warm-up first, the two paths alternating inside every repetition),
  * the fused pass alone (pp_dose_histogram_f32: every structure's histogram and statistics from one pass),
  * the whole pa.dose.dvh_table call (it resamples the dose onto the first label's grid first, as the reference does) and
  * pa.dose.calculate_d_to_volume (D2 of the largest structure)
against the same results COMPOSED from torch ops on the GPU: per structure boolean indexing, torch.bucketize on the same fp64
edges, torch.bincount, sum / min / max -- and one torch.sort of the indexed values for the percentile.  The composed counts must EQUAL the
kernel's: that is the tool's correctness check.  Also prints the bytes per voxel the fused pass asks memory for (every mask
byte, and the 128-byte dose lines that hold a voxel of some structure) beside the compulsory 4 + L.
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
from platipy_amd.registration.utils import resample_image  # noqa: E402


def phantom(size, nstruct, device):
    """A dose of a few overlapping Gaussian beams (0 ... ~70 Gy) with 0.5 % noise, and ellipsoids whose volumes are spread
    geometrically between 0.1 % and 5 % of the grid."""
    nx, ny, nz = size
    g = torch.Generator(device="cpu").manual_seed(11)
    z, y, x = torch.meshgrid(torch.arange(nz, device=device, dtype=torch.float32) / nz, torch.arange(ny, device=device, dtype=torch.float32) / ny,
                             torch.arange(nx, device=device, dtype=torch.float32) / nx, indexing="ij")
    dose = torch.zeros((nz, ny, nx), device=device)
    for _ in range(3):
        c = (0.35 + 0.3 * torch.rand(3, generator=g)).tolist()
        s = (0.12 + 0.1 * torch.rand(3, generator=g)).tolist()
        dose += 30.0 * torch.exp(-(((x - c[0]) / s[0]) ** 2 + ((y - c[1]) / s[1]) ** 2 + ((z - c[2]) / s[2]) ** 2))
    dose *= 1.0 + 0.005 * torch.randn((nz, ny, nx), generator=g).to(device)
    masks = {}
    for k, frac in enumerate(np.geomspace(0.001, 0.05, nstruct)):
        a = (3.0 * frac / (4.0 * math.pi)) ** (1.0 / 3.0)
        c = (a + (1.0 - 2.0 * a) * torch.rand(3, generator=g)).tolist()
        masks[f"structure_{k}"] = ((((x - c[0]) / a) ** 2 + ((y - c[1]) / a) ** 2 + ((z - c[2]) / a) ** 2) <= 1.0).to(torch.uint8).contiguous()
    return dose.contiguous(), masks


def composed_tables(dose, masks, edges):
    """Per structure: counts (np.histogram's rule), voxel count, mask sum, fp64 dose sum, min, max -> stacked, on the host."""
    nbins = edges.numel() - 1
    flat = dose.reshape(-1)
    counts, stats = [], []
    for m in masks:
        mf = m.reshape(-1)
        vals = flat[mf != 0]
        v64 = vals.double()
        idx = (torch.bucketize(v64, edges, right=True) - 1).clamp_(max=nbins - 1)
        keep = (v64 >= edges[0]) & (v64 <= edges[-1])
        counts.append(torch.bincount(idx[keep], minlength=nbins))
        stats.append(torch.stack([torch.tensor(float(vals.numel()), dtype=torch.float64, device=dose.device), mf.sum().double(), v64.sum(),
                                  vals.min().double(), vals.max().double()]))
    return torch.stack(counts).cpu().numpy(), torch.stack(stats).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--structures", type=int, default=8)
    ap.add_argument("--bin-width", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "dvh_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "dvh_bench needs a GPU"
    dev = torch.device("cuda", 0)
    spacing = (0.98, 0.98, 2.5)
    dose_t, mask_t = phantom(a_.size, a_.structures, dev)
    dose = pa.Image(dose_t, spacing)
    labels = {k: pa.Image(v, spacing) for k, v in mask_t.items()}
    masks = list(mask_t.values())
    n, nl = dose_t.numel(), len(masks)
    ctx = runtime.context(dev)
    max_dose = float(dose_t.max())
    edges = np.arange(-a_.bin_width / 2, max_dose + a_.bin_width, a_.bin_width)
    edges_t = torch.from_numpy(edges).to(dev)
    first = labels[next(iter(labels))]
    biggest = list(labels)[-1]

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def quantile_new():
        return float(pa.dose.calculate_d_to_volume(dose, labels[biggest], 2))

    def quantile_old():
        vals = resample_image(dose, labels[biggest]).tensor.reshape(-1)[labels[biggest].tensor.reshape(-1) > 0]
        # (torch.quantile places the rank in fp32: at 3 M values its weight is off by a quarter of a rank; one sort and
        # numpy's interpolation between the two neighbours instead)
        srt = torch.sort(vals).values
        virtual = (vals.numel() - 1) * 0.98
        below = int(math.floor(virtual))
        a, b = srt[below].item(), srt[min(below + 1, vals.numel() - 1)].item()
        t = float(np.float32(virtual - below))
        return float(np.float32(b - (b - a) * (1 - t)) if t >= 0.5 else np.float32(a + (b - a) * t))

    cases = {
        "histogram_kernel": (lambda: ctx.dose_histogram(dose_t, masks, n, edges), lambda: composed_tables(dose_t, masks, edges_t)),
        "dvh_table": (lambda: pa.dose.dvh_table(dose, labels, bin_width=a_.bin_width),
                      lambda: composed_tables(resample_image(dose, first).tensor, masks, edges_t)),
        "d_to_volume": (quantile_new, quantile_old),
    }
    any_mask = torch.zeros(n, dtype=torch.bool, device=dev)
    for m in masks:
        any_mask |= m.reshape(-1) != 0
    lines = any_mask[: n // 32 * 32].reshape(-1, 32).any(dim=1).double().mean().item()     # 128-byte dose lines with a structure voxel
    result = {"size": a_.size, "spacing": spacing, "structures": nl, "bins": int(edges.size - 1), "reps": a_.reps,
              "structure_fraction": [round(float((m != 0).double().mean()), 5) for m in masks],
              "bytes_per_voxel_compulsory": 4 + nl, "bytes_per_voxel_requested": round(nl + 4 * lines, 3)}
    for name, (new, old) in cases.items():
        for _ in range(2):                      # warm-up (and the values)
            vn, vo = new(), old()
        if name == "histogram_kernel":
            assert np.array_equal(vn[0], vo[0]), "the composed counts differ from the kernel's"
            assert np.array_equal(vn[1]["count"], vo[1][:, 0]) and np.array_equal(vn[1]["mask_sum"], vo[1][:, 1])
            assert np.array_equal(vn[1]["dose_min"], vo[1][:, 3]) and np.array_equal(vn[1]["dose_max"], vo[1][:, 4])
            np.testing.assert_allclose(vn[1]["dose_sum"], vo[1][:, 2], rtol=1e-12)
            check = {"counts_equal": True, "voxels_counted": int(vn[0].sum())}
        elif name == "dvh_table":
            assert np.array_equal(vn.counts, vo[0]), "the composed counts differ from dvh_table's"
            check = {"counts_equal": True}
        else:
            assert abs(vn - vo) <= 4 * float(np.spacing(np.float32(max(abs(vn), abs(vo))))), (vn, vo)
            check = {"value": vn, "composed_value": vo}
        tn, to = [], []
        for _ in range(a_.reps):
            tn.append(event_ms(new)[0])
            to.append(event_ms(old)[0])
        result[name] = {"new_ms_median": round(statistics.median(tn), 3), "new_ms_min": round(min(tn), 3),
                        "new_ms_spread": round(max(tn) - min(tn), 3), "composed_ms_median": round(statistics.median(to), 3),
                        "composed_ms_min": round(min(to), 3), "composed_ms_spread": round(max(to) - min(to), 3),
                        "composed_over_new": round(statistics.median(to) / statistics.median(tn), 2), **check}
    result["histogram_kernel"]["compulsory_GB_per_s"] = round((4 + nl) * n / (result["histogram_kernel"]["new_ms_median"] * 1e-3) / 1e9, 1)
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
