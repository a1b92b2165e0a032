"""Timings of the SIFT landmark kernels (csrc/pp_sift.h) on a GPU, HIP events, medians of --reps, at 256 x 256 x 128 and
512 x 512 x 256 isotropic voxels of the seeded CT phantom plus a seeded texture (white noise blurred to sigma 2 voxels, about
60 HU), clamped to the window [-200, 300] that also normalises the contrast threshold:

  * pp_dog_extrema_f32 on the first octave's stack (intervals + 3 = 6 Gaussian volumes): ms of the whole call (its three
    passes, the read-back of the count and of the rows) and GB/s of its compulsory reads, 6 x 4 bytes per voxel; against
    the SAME candidates composed from torch: max_pool3d (3 x 3 x 3, stride 1) of the stacked differences and of their
    negatives, compared across adjacent levels, ties among the survivors removed by a gather of their 26 neighbours.  The
    two candidate sets are compared in the same run.  The kept keypoints (refinement and tests) are timed as well: the
    composition has no counterpart for them.
  * pp_sift_describe_f32: ms per 1 000 keypoints.
  * pp_descriptor_match_f32 on 4 000 x 4 000 descriptors of length 768 against torch.cdist + topk(2); partners compared in
    the same run wherever best and second differ by more than the fp32 accumulation bound.
  * sift_keypoints as a whole, wall clock, and the share of it spent in scale_space (the existing Gaussian passes).

  python tools/sift_bench.py --out profiles/sift_bench.json"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import platipy_amd as pa  # noqa: E402
from augment_bench import phantom  # noqa: E402  (the same seeded phantom, not a copy)
from platipy_amd.registration import qa as Q  # noqa: E402


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


def wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def composed_candidates(stack):
    """S3 from torch -> int64 keys ((level nz + z) ny + y) nx + x of the candidates, ascending."""
    F = torch.nn.functional
    d = stack[1:] - stack[:-1]                                  # [levels - 1, Z, Y, X]
    nl, nz, ny, nx = d.shape
    keys = []
    for sign in (1.0, -1.0):
        v = d * sign
        m = F.max_pool3d(v[None], 3, stride=1, padding=1)[0]    # the 27-neighbourhood maximum on every level, the centre included
        c = (v[1:-1] == m[1:-1]) & (v[1:-1] > m[:-2]) & (v[1:-1] > m[2:])
        c[:, 0], c[:, -1], c[:, :, 0], c[:, :, -1], c[:, :, :, 0], c[:, :, :, -1] = False, False, False, False, False, False
        l, z, y, x = torch.nonzero(c, as_tuple=True)
        l = l + 1
        tie = torch.zeros_like(l, dtype=torch.bool)             # a non-strict maximum: drop it when a neighbour on its level equals it
        centre = v[l, z, y, x]
        for k in range(27):
            if k == 13:
                continue
            dz, dy, dx = k // 9 - 1, (k // 3) % 3 - 1, k % 3 - 1
            tie |= v[l, z + dz, y + dy, x + dx] == centre
        keep = ~tie
        keys.append(((l[keep] * nz + z[keep]) * ny + y[keep]) * nx + x[keep])
    return torch.sort(torch.cat(keys))[0]


def bench_size(size, reps):
    dev = torch.device("cuda", 0)
    ct, _ = phantom(size, 2, dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    ctx = pa.runtime.context(dev)
    # texture: white noise blurred to sigma 2 voxels, about 60 HU, so that blobs of keypoint size and contrast exist
    tex = (1100.0 * torch.randn(ct.shape, generator=g)).to(dev).contiguous()
    blurred = torch.empty_like(tex)
    ctx.discrete_gaussian(tex, blurred, size, (1.0, 1.0, 1.0), [4.0] * 3, 0.01, 32, True)
    lo, hi = -200.0, 300.0                                      # the window, as dir_qa clamps to one
    ct = (ct + blurred).clamp(lo, hi).contiguous()
    del tex, blurred
    image = pa.Image(ct, (1.0, 1.0, 1.0))
    n = ct.numel()
    octave = Q.scale_space(image, 1, 3, None)[0]
    stack, sz, nlev = octave["stack"], octave["size"], int(octave["stack"].shape[0])
    count_c, index_c, _ = ctx.dog_extrema(stack, sz, nlev, hi - lo, 0.03, 172.3, 0, candidates_only=True)
    count_c, index_c, _ = ctx.dog_extrema(stack, sz, nlev, hi - lo, 0.03, 172.3, count_c, candidates_only=True)
    t_cand = median_ms(lambda: ctx.dog_extrema(stack, sz, nlev, hi - lo, 0.03, 172.3, count_c, candidates_only=True), reps)
    count_k, index_k, _ = ctx.dog_extrema(stack, sz, nlev, hi - lo, 0.03, 172.3, 0)
    t_kept = median_ms(lambda: ctx.dog_extrema(stack, sz, nlev, hi - lo, 0.03, 172.3, count_k), reps)
    _, index_k, _ = ctx.dog_extrema(stack, sz, nlev, hi - lo, 0.03, 172.3, count_k)
    t_comp = median_ms(lambda: composed_candidates(stack).cpu(), reps)
    want = composed_candidates(stack).cpu().numpy()
    i = index_c.astype(np.int64)
    got = ((i[:, 3] * sz[2] + i[:, 2]) * sz[1] + i[:, 1]) * sz[0] + i[:, 0]
    equal = bool(np.array_equal(got, want))
    assert equal, f"{size}: the composed candidates differ from the kernel's ({len(got)} against {len(want)})"
    nd = min(len(index_k), 4000)
    t_desc = None
    if nd:
        desc = torch.empty((nd, 768), dtype=torch.float32, device=dev)
        t_desc = median_ms(lambda: ctx.sift_describe(stack, sz, nlev, octave["spacing"], index_k[:nd], desc), reps)
    t_space = wall_ms(lambda: Q.scale_space(image, 3, 3, None), reps)
    t_all = wall_ms(lambda: Q.sift_keypoints(image, intensity_range=(lo, hi)), reps)
    kp = Q.sift_keypoints(image, intensity_range=(lo, hi))
    gb = nlev * 4 * n / 1e9
    return {"size": list(size), "voxels": n, "levels": nlev, "candidates": int(count_c), "kept": int(count_k),
            "extrema_candidates_ms": round(t_cand, 3), "extrema_candidates_GB_per_s": round(gb / (t_cand * 1e-3), 1),
            "extrema_kept_ms": round(t_kept, 3), "extrema_kept_GB_per_s": round(gb / (t_kept * 1e-3), 1),
            "composed_candidates_ms": round(t_comp, 3), "composed_over_kernel": round(t_comp / t_cand, 2), "candidates_equal": equal,
            "describe_keypoints": nd, "describe_ms_per_1000": None if t_desc is None else round(1000.0 * t_desc / nd, 3),
            "sift_keypoints_wall_ms": round(t_all, 2), "scale_space_wall_ms": round(t_space, 2),
            "gaussian_share": round(t_space / t_all, 3), "keypoints": len(kp)}


def bench_match(reps, n=4000, length=768):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(11)
    a, b = (torch.rand((n, length), generator=g) ** 3).to(dev), (torch.rand((n, length), generator=g) ** 3).to(dev)
    a, b = (a / a.norm(dim=1, keepdim=True)).contiguous(), (b / b.norm(dim=1, keepdim=True)).contiguous()
    ctx = pa.runtime.context(dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    best, second = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    t_k = median_ms(lambda: ctx.descriptor_match(a, n, b, n, length, idx, best, second), reps)

    def composed():
        d = torch.cdist(a, b)
        return torch.topk(d, 2, dim=1, largest=False)
    t_c = median_ms(composed, reps)
    val, ind = composed()
    torch.cuda.synchronize()
    bound = 1.01 * (length + 2) * 2.0 ** -24 * best.double()
    clear = (second.double() - best.double()) > 4 * bound
    equal = bool((idx[clear].long() == ind[clear, 0]).all()) and bool(((val[:, 0].double() ** 2 - best.double()).abs() <= 1e-4 * best.double() + 1e-6).all())
    assert equal, "the composed partners differ from the kernel's"
    return {"rows_a": n, "rows_b": n, "length": length, "match_ms": round(t_k, 3), "cdist_topk_ms": round(t_c, 3),
            "composed_over_kernel": round(t_c / t_k, 2), "rows_compared": int(clear.sum()), "partners_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 256, 128, 512, 512, 256], help="NX NY NZ, one triple per volume")
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "sift_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "sift_bench needs a GPU"
    sizes = [tuple(a_.sizes[k:k + 3]) for k in range(0, len(a_.sizes), 3)]
    result = {"reps": a_.reps, "volumes": [bench_size(s, a_.reps) for s in sizes], "match": bench_match(a_.reps)}
    line = json.dumps(result)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
