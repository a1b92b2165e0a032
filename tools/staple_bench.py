#!/usr/bin/env python
"""STAPLE (pp_staple_fuse) at the size of a planning CT: 512 x 512 x 256 voxels, 16 uint8 raters made from one smooth
structure (per-rater shifts and erosions plus sparse flips; tests/staple_restatement.raters_from_truth).

Prints one JSON line: end-to-end ms of platipy_amd.label.staple and combine_labels_staple (device-synchronised, median
of --reps), per-phase HIP-event ms of one profiled call, the iteration count and the mixed-voxel fraction."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import platipy_amd as pa  # noqa: E402
from platipy_amd import _lib, runtime  # noqa: E402
from tests.staple_restatement import raters_from_truth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--raters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=31)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "staple_bench needs a GPU"
    dev = torch.device("cuda", 0)
    nx, ny, nz = a.size
    labels = [pa.image_from_array(x, device=dev) for x in raters_from_truth((nz, ny, nx), a.raters, a.seed)]
    ctx = runtime.context(dev)

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts)

    st_med, st_min = timed(lambda: pa.label.staple(labels))
    cb_med, cb_min = timed(lambda: pa.label.combine_labels_staple({i: {"s": x} for i, x in enumerate(labels)}))

    n = labels[0].tensor.numel()
    out = torch.empty(labels[0].tensor.shape, dtype=torch.float64, device=dev)
    ctx.profile_enable(True)
    ctx.profile_read()
    res = ctx.staple([x.tensor for x in labels], False, n, out, _lib.STAPLE_FOREGROUND)
    phases = {k: {"launches": v[0], "ms": round(v[1], 4)} for k, v in ctx.profile_read().items()}
    ctx.profile_enable(False)
    print(json.dumps({
        "size": a.size, "raters": a.raters, "reps": a.reps,
        "staple_ms_median": round(st_med, 3), "staple_ms_min": round(st_min, 3),
        "combine_labels_staple_ms_median": round(cb_med, 3), "combine_labels_staple_ms_min": round(cb_min, 3),
        "iterations": int(res.elapsed_iterations), "mixed_fraction": round(res.n_mixed / n, 5),
        "n_zero": int(res.n_zero), "n_one": int(res.n_one), "n_mixed": int(res.n_mixed),
        "phases_profiled_call": phases,
        "phases_sum_ms": round(sum(v["ms"] for v in phases.values()), 4),
    }))


if __name__ == "__main__":
    main()
