"""Time the two B-spline kernels at 512 x 512 x 256 (1 mm), meshes 8 x 8 x 4 and 32 x 32 x 16, against the same quantities
composed from torch: separable einsum evaluation of the field; grid_sample + index_add_ for the mean-squares gradient.  Beside
the mean-squares evaluation: the two passes of Mattes mutual information (30 bins) and one whole evaluation (histogram pass,
the host's score table, gradient pass), with their ratio to the mean-squares evaluation of the same run.  --baseline-lib PATH
times the mean-squares evaluation of another build of the library (the parent commit's, say) in the same run on the same box.

HIP-event times, medians over --repeats after --warmup launches, buffers allocated once, a 512 MB scrub between timed launches
so no launch starts with its inputs in Infinity Cache.  Writes profiles/bspline_bench.json; the bytes/voxel "requested" beside the compulsory bytes are modelled from the access
pattern, not read from counters.  For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python
tools/bspline_bench.py --repeats 3` and keep the stats file beside the JSON."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import platipy_amd as pa  # noqa: E402
from platipy_amd import _lib, runtime  # noqa: E402
from platipy_amd.registration import _mattes  # noqa: E402

SIZE = (512, 512, 256)


def timed(fn, warmup, repeats, scrub):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        scrub.add_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [float(t) for t in times]


def load_baseline(path):
    """Another build of the library, which may predate entry points this one has: what it exports is declared, the rest is left out."""
    dll = ctypes.CDLL(path)
    for name, (res, argtypes) in _lib._SIGNATURES.items():
        if hasattr(dll, name):
            fn = getattr(dll, name)
            fn.restype, fn.argtypes = res, argtypes
    return dll


def basis(t):
    return torch.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6], -1)


def axis_matrix(n, mesh, dev):
    """[n, mesh + 3]: weights of the lattice's control points at the n voxel centres of an axis the domain spans"""
    u = (torch.arange(n, device=dev, dtype=torch.float64) + 0.5) * (mesh / n) + 1.0
    fl = torch.floor(u)
    w = basis(u - fl)
    W = torch.zeros((n, mesh + 3), device=dev, dtype=torch.float64)
    for q in range(4):
        W.scatter_add_(1, (fl.long() - 1 + q)[:, None], w[:, q:q + 1])
    return W.float()


def separable_field(Wz, Wy, Wx, coef):
    """the dense field, one axis at a time (a single four-operand einsum picks a contraction order that does not fit in memory)"""
    a = torch.einsum("xi,ckji->ckjx", Wx, coef)
    a = torch.einsum("yj,ckjx->ckyx", Wy, a)
    return torch.einsum("zk,ckyx->czyx", Wz, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "bspline_bench.json"))
    ap.add_argument("--baseline-lib", default=None, help="another build of libplatipy_hip.so whose mean-squares evaluation is timed beside this one's")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = runtime.context(dev)
    base_ctx = None
    if args.baseline_lib:
        base_ctx = _lib.Context(0, torch.cuda.current_stream().cuda_stream, lib=load_baseline(args.baseline_lib))
    g = torch.Generator(device="cpu").manual_seed(1)
    fixed = torch.randn(SIZE[::-1], generator=g).to(dev)
    moving = torch.randn(SIZE[::-1], generator=g).to(dev)
    img = pa.Image(fixed, (1.0, 1.0, 1.0))
    geom = img.geom()
    scrub = torch.zeros(128 << 20, device=dev)
    field = torch.empty((3,) + SIZE[::-1], device=dev)
    nvox = float(np.prod(SIZE))
    result = {"size": SIZE, "spacing": 1.0, "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
              "cases": []}
    bins = _mattes.make_bins(30, _lib.MI_MATTES, (float(fixed.min()), float(fixed.max())), (float(moving.min()), float(moving.max())))
    for mesh in ((8, 8, 4), (32, 32, 16)):
        t = pa.bspline_transform_initializer(img, mesh)
        t.SetParameters(np.random.default_rng(2).normal(0, 2.0, t.GetNumberOfParameters()))
        lg = t.lattice_geom()
        case = {"mesh": mesh, "parameters": t.GetNumberOfParameters()}
        ms, all_ms = timed(lambda: ctx.bspline_field(t.coefficients, lg, geom, field), args.warmup, args.repeats, scrub)
        case["field_ms"], case["field_ms_all"] = ms, all_ms
        # "requested_modelled" is arithmetic on the kernel's access pattern, not a hardware counter
        case["field_bytes_per_voxel"] = {"compulsory": 12.0, "requested_modelled": 12.0 + 4.0 * t.GetNumberOfParameters() / nvox,
                                         "achieved_GBps": 12.0 * nvox / ms / 1e6}
        Wx, Wy, Wz = (axis_matrix(SIZE[a], mesh[a], dev) for a in range(3))
        ms, all_ms = timed(lambda: separable_field(Wz, Wy, Wx, t.coefficients), args.warmup, args.repeats, scrub)
        case["field_torch_einsum_ms"] = ms
        for rate in (0.1, 1.0):
            stride = int(np.ceil(1.0 / rate)) if rate < 1.0 else 1
            fn = lambda: ctx.bspline_metric(_lib.BSPLINE_MEAN_SQUARES, fixed, geom, moving, geom, geom, stride, t.coefficients, lg)  # noqa: E731
            ms, all_ms = timed(fn, args.warmup, args.repeats, scrub)
            nsamp = nvox / stride
            case[f"metric_rate_{rate}_ms"] = ms
            case[f"metric_rate_{rate}_bytes_per_sample"] = {"compulsory": 8.0, "requested_modelled": 4.0 * 8 + 4.0 * 8,
                                                            "note": "modelled, not counted: 8 trilinear corners of each image; neighbours share cache lines"}
            case[f"metric_rate_{rate}_samples_per_us"] = nsamp / ms / 1e3
            case[f"metric_rate_{rate}_ms_all"] = all_ms
            if base_ctx is not None:
                fn = lambda: base_ctx.bspline_metric(_lib.BSPLINE_MEAN_SQUARES, fixed, geom, moving, geom, geom, stride, t.coefficients, lg)  # noqa: E731
                case[f"metric_rate_{rate}_baseline_ms"], case[f"metric_rate_{rate}_baseline_ms_all"] = timed(fn, args.warmup, args.repeats, scrub)
            # Mattes mutual information, 30 bins: pass 1, pass 2 (on the table of pass 1's histogram) and a whole evaluation
            margs = (fixed, geom, moving, geom, geom, stride, t.coefficients, lg, bins)
            hist, st = ctx.bspline_mi_histogram(*margs)
            table = _mattes.value_and_table("mattes_mi", hist, st["valid"], bins.m_bin)[1]

            def evaluation():
                h, s_ = ctx.bspline_mi_histogram(*margs)
                return ctx.bspline_mi_gradient(*margs, _mattes.value_and_table("mattes_mi", h, s_["valid"], bins.m_bin)[1])

            for key, fn in (("mi_histogram", lambda: ctx.bspline_mi_histogram(*margs)), ("mi_gradient", lambda: ctx.bspline_mi_gradient(*margs, table)),
                            ("mi_evaluation", evaluation)):
                case[f"{key}_rate_{rate}_ms"], case[f"{key}_rate_{rate}_ms_all"] = timed(fn, args.warmup, args.repeats, scrub)
                case[f"{key}_rate_{rate}_over_mean_squares"] = case[f"{key}_rate_{rate}_ms"] / ms
        # torch composition of one mean-squares value + gradient on every stride-th voxel: field by einsum, grid_sample (value, and
        # the spatial gradient by autograd through the sampling positions), then index_add_ of the 64 weighted terms per sample
        def torch_metric(stride):
            disp = separable_field(Wz, Wy, Wx, t.coefficients).reshape(3, -1)
            lin = torch.arange(0, int(nvox), stride, device=dev)
            x, y, z = lin % SIZE[0], (lin // SIZE[0]) % SIZE[1], lin // (SIZE[0] * SIZE[1])
            d = disp[:, lin]
            pos = torch.stack([(x + d[0]) / (SIZE[0] - 1), (y + d[1]) / (SIZE[1] - 1), (z + d[2]) / (SIZE[2] - 1)], -1) * 2 - 1
            pos.requires_grad_(True)
            m = torch.nn.functional.grid_sample(moving[None, None], pos[None, None, None], mode="bilinear", align_corners=True).reshape(-1)
            value = ((fixed.reshape(-1)[lin] - m) ** 2).mean()
            (gpos,) = torch.autograd.grad(value, pos)
            grad = torch.zeros_like(t.coefficients).reshape(3, -1)
            fx = ((x + 0.5) * mesh[0] / SIZE[0]).floor().long()
            fy = ((y + 0.5) * mesh[1] / SIZE[1]).floor().long()
            fz = ((z + 0.5) * mesh[2] / SIZE[2]).floor().long()
            cx, cy = mesh[0] + 3, mesh[1] + 3
            for k in range(4):
                wz_ = Wz[z, fz + k]
                for j in range(4):
                    wyz = wz_ * Wy[y, fy + j]
                    for i in range(4):
                        w = wyz * Wx[x, fx + i]
                        cp = ((fz + k) * cy + (fy + j)) * cx + (fx + i)
                        for r in range(3):
                            grad[r].index_add_(0, cp, gpos[:, r] * w)
            return value, grad

        for rate in (0.1, 1.0):
            stride = int(np.ceil(1.0 / rate)) if rate < 1.0 else 1
            ms, all_ms = timed(lambda: torch_metric(stride), 1, max(2, args.repeats // 3), scrub)
            case[f"metric_rate_{rate}_torch_ms"] = ms
        result["cases"].append(case)
        print(json.dumps(case))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
