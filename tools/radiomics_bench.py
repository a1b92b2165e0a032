#!/usr/bin/env python
"""Radiomics tables at the size of a planning CT: a seeded 512 x 512 x 256 fp32 phantom, spacing (0.98, 0.98, 2.5), and 8
uint8 ellipsoid structures of 0.1 % ... 5 % of the grid (the phantom of tools/augment_bench.py), binWidth 25.

Per structure, on the crop of its bounding box, with HIP events (warm-up first, medians of --reps; every call includes its
own read-back of the tables, as the library makes it):
  * pp_radiomics_discretise_f32          compulsory bytes: 5 B per voxel of the box (4 read + 1 mask read; the 2 B written
                                         are reported apart)
  * pp_texture_neighbourhood_u16         all of GLCM, GLDM and NGTDM in one pass: 2 B per voxel
  * pp_texture_runs_u16                  2 B per voxel
and the same tables COMPOSED FROM TORCH in the same run, results asserted equal: the GLCM from shifted slices and
torch.bincount on (a - 1) Ng + (b - 1) per direction; GLDM and NGTDM from 26 shifted views of the zero-padded levels
(neighbour counts, same-level counts and level sums) and three bincounts.  No composition is offered for the runs: a maximal
run has no reasonable form in shifted slices.  Also the wall clock of one pa.radiomics.extract_radiomics call with every
class for all structures.  Prints one JSON line; --out writes it to a file.

The plain phantom is smooth inside a structure (3 ... 6 grey levels at binWidth 25: the most contended end of the LDS
counters, one GLCM direction group).  --texture-sd SD adds seeded Gaussian noise of SD image units, which spreads a structure
over about 8 ... 10 SD / binWidth levels, as texture does in a CT structure: SD 120 keeps every table in LDS with the GLCM
in several direction groups (profiles/radiomics_bench_sd120.json), SD 250 lies on both sides of the thresholds to global
atomics (profiles/radiomics_bench_sd250.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import platipy_amd as pa  # noqa: E402
from augment_bench import phantom  # noqa: E402  (the same seeded phantom, not a copy)
from platipy_amd import radiomics as R  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def median_ms(fn, reps):
    fn()
    return statistics.median(event_ms(fn)[0] for _ in range(reps))


def composed_glcm(L, ng):
    out = []
    nz, ny, nx = L.shape
    for c in range(14, 27):
        dz, dy, dx = c // 9 - 1, (c // 3) % 3 - 1, c % 3 - 1
        def sl(n, d):
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (za, zb), (ya, yb), (xa, xb) = sl(nz, dz), sl(ny, dy), sl(nx, dx)
        a, b = L[za, ya, xa], L[zb, yb, xb]
        valid = (a > 0) & (b > 0)
        out.append(torch.bincount(((a - 1) * ng + (b - 1))[valid], minlength=ng * ng).reshape(ng, ng))
    return torch.stack(out)


def composed_neighbour_tables(L, ng):
    P = torch.nn.functional.pad(L, (1, 1, 1, 1, 1, 1))
    nz, ny, nx = L.shape
    k, dep, total = torch.zeros_like(L), torch.zeros_like(L), torch.zeros_like(L)
    for c in range(27):
        if c == 13:
            continue
        dz, dy, dx = c // 9, (c // 3) % 3, c % 3
        nb = P[dz:dz + nz, dy:dy + ny, dx:dx + nx]
        k += nb > 0
        dep += (nb == L) & (nb > 0)
        total += nb
    inside = L > 0
    row = (L[inside] - 1) * 27
    gldm = torch.bincount(row + dep[inside], minlength=27 * ng).reshape(ng, 27)
    n = torch.bincount(row + k[inside], minlength=27 * ng).reshape(ng, 27)
    s = torch.bincount(row + k[inside], weights=(L * k - total)[inside].abs().double(), minlength=27 * ng).reshape(ng, 27).long()
    return gldm, n, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--structures", type=int, default=8)
    ap.add_argument("--bin-width", type=float, default=25.0)
    ap.add_argument("--texture-sd", type=float, default=0.0, help="sd of seeded Gaussian noise added to the phantom (0: none)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "radiomics_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "radiomics_bench needs a GPU"
    dev = torch.device("cuda", 0)
    spacing = (0.98, 0.98, 2.5)
    ct_t, mask_t = phantom(a_.size, a_.structures, dev)
    if a_.texture_sd > 0.0:
        g = torch.Generator(device="cpu").manual_seed(12)
        ct_t = (ct_t + a_.texture_sd * torch.randn(ct_t.shape, generator=g).to(dev)).contiguous()
    ct = pa.Image(ct_t, spacing)
    masks = {f"s{k}": pa.Image(m, spacing) for k, m in enumerate(mask_t)}
    bw = a_.bin_width
    per = []
    tot = {"box_voxels": 0, "discretise_ms": 0.0, "neighbourhood_ms": 0.0, "runs_ms": 0.0, "composed_glcm_ms": 0.0, "composed_gldm_ngtdm_ms": 0.0}
    for name, mask in masks.items():
        s = R._Structure(ct, mask, name)
        e = s.edges(bw)
        lev, ng, _ = s.levels(bw)
        ctx, n = s.ctx, s.n
        t_disc = median_ms(lambda: ctx.radiomics_discretise(s.image, s.mask, n, e, lev), a_.reps)
        t_nb = median_ms(lambda: ctx.texture_neighbourhood(lev, s.size, ng), a_.reps)
        t_runs = median_ms(lambda: ctx.texture_runs(lev, s.size, ng), a_.reps)
        L = (lev.long() & 0xFFFF)
        got = ctx.texture_neighbourhood(lev, s.size, ng)
        t_cg = median_ms(lambda: composed_glcm(L, ng).cpu(), a_.reps)
        t_cn = median_ms(lambda: [t.cpu() for t in composed_neighbour_tables(L, ng)], a_.reps)
        cg = composed_glcm(L, ng).cpu().numpy()
        cd, cn, cs = (t.cpu().numpy() for t in composed_neighbour_tables(L, ng))
        equal = bool((cg == got["glcm"]).all() and (cd == got["gldm"]).all() and (cn == got["ngtdm_n"]).all() and (cs == got["ngtdm_s"]).all())
        assert equal, f"{name}: the composed tables differ from the kernel's"
        per.append({"structure": name, "box": list(s.size), "box_voxels": n, "voxels_inside": s.count, "ng": ng,
                    "discretise_ms": round(t_disc, 3), "discretise_GB_per_s": round(5 * n / (t_disc * 1e-3) / 1e9, 1),
                    "neighbourhood_ms": round(t_nb, 3), "neighbourhood_GB_per_s": round(2 * n / (t_nb * 1e-3) / 1e9, 1),
                    "runs_ms": round(t_runs, 3), "runs_GB_per_s": round(2 * n / (t_runs * 1e-3) / 1e9, 1),
                    "composed_glcm_ms": round(t_cg, 3), "composed_gldm_ngtdm_ms": round(t_cn, 3),
                    "composed_over_kernel": round((t_cg + t_cn) / t_nb, 2), "tables_equal": equal})
        tot["box_voxels"] += n
        for k, v in (("discretise_ms", t_disc), ("neighbourhood_ms", t_nb), ("runs_ms", t_runs), ("composed_glcm_ms", t_cg),
                     ("composed_gldm_ngtdm_ms", t_cn)):
            tot[k] += v
        del L, cg, cd, cn, cs
    every = {rad: list(names) for rad, names in R.features.FEATURES.items()}
    R.extract_radiomics(ct, masks, radiomics=every, pyradiomics_settings={"binWidth": bw})
    wall = []
    for _ in range(a_.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        R.extract_radiomics(ct, masks, radiomics=every, pyradiomics_settings={"binWidth": bw})
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    nv = tot["box_voxels"]
    result = {"size": a_.size, "spacing": spacing, "structures": len(masks), "bin_width": bw, "texture_sd": a_.texture_sd, "reps": a_.reps,
              "totals": {**{k: (round(v, 3) if isinstance(v, float) else v) for k, v in tot.items()},
                         "discretise_GB_per_s": round(5 * nv / (tot["discretise_ms"] * 1e-3) / 1e9, 1),
                         "neighbourhood_GB_per_s": round(2 * nv / (tot["neighbourhood_ms"] * 1e-3) / 1e9, 1),
                         "runs_GB_per_s": round(2 * nv / (tot["runs_ms"] * 1e-3) / 1e9, 1),
                         "composed_over_kernel": round((tot["composed_glcm_ms"] + tot["composed_gldm_ngtdm_ms"]) / tot["neighbourhood_ms"], 2)},
              "extract_radiomics_all_classes_wall_ms_median": round(statistics.median(wall), 2),
              "extract_radiomics_all_classes_wall_ms_min": round(min(wall), 2), "per_structure": per}
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
