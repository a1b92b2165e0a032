#!/usr/bin/env python
"""Masks to RTSTRUCT contours at the size of a planning CT: 512 x 512 x 256, 24 structures.

The input is the seeded phantom of tools/contour_bench.py (ellipsoids, every third one a ring), rasterised by
pp_contour_fill_u8; pp_contour_trace_u8 then extracts the contours of all structures and slices in one go.

Times, with HIP events (warm-up first, medians of 5),
  * the whole extraction as Context.contour_trace makes it: count call, fill call, the copy of the tables to the host;
  * its stages, by the library's own event brackets (Context.profile_enable): the counting stream pass, the table scan, the
    emitting stream pass, the successors, the leader rounds, the ranking rounds, the output stage, the copy-out;
  * pp_slice_contour_u8 over the same bytes in the same run: a streaming byte kernel that reads every voxel once and writes
    one byte per voxel, the yardstick for the two stream passes.
GB/s counts the compulsory read of 1 byte per voxel and structure.  The round trip is checked in the same run: filling the
extracted contours must give the masks back byte for byte.  No composition of contour tracing from torch operators exists
and none is invented here.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from contour_bench import phantom  # noqa: E402  (the same seeded phantom, not a copy)
from platipy_amd import runtime  # noqa: E402

STAGES = (("k_tr_stream_count", "stream_count"), ("tr_table_scan", "table_scan"), ("k_tr_stream_emit", "stream_emit"), ("k_tr_succ", "successors"),
          ("tr_leader_rounds", "leader_rounds"), ("tr_rank_rounds", "rank_rounds"), ("tr_output", "output"), ("tr_copy_out", "copy_out"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=[512, 512, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--structures", type=int, default=24)
    ap.add_argument("--vertices", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20240611)
    ap.add_argument("--out", nargs="?", const=os.path.join(ROOT, "profiles", "contour_trace_bench.json"), default=None)
    a_ = ap.parse_args()
    assert torch.cuda.is_available(), "contour_trace_bench needs a GPU"
    dev = torch.device("cuda", 0)
    nx, ny, nz = a_.size
    S = a_.structures
    ctx = runtime.context(dev)
    pverts, ptable, _ = phantom(a_.size, S, a_.vertices, a_.seed)
    masks = torch.empty((S, nz, ny, nx), dtype=torch.uint8, device=dev)
    ctx.contour_fill(pverts, ptable, a_.size, S, masks)
    back = torch.empty_like(masks)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def stats(t, nbytes=None):
        m = statistics.median(t)
        d = {"ms_median": round(m, 3), "ms_min": round(min(t), 3), "ms_spread": round(max(t) - min(t), 3)}
        if nbytes:
            d["read_GB_per_s"] = round(nbytes / (m * 1e-3) / 1e9, 1)
        return d

    nbytes = masks.numel()
    result = {"size": a_.size, "structures": S, "reps": a_.reps, "seed": a_.seed, "inside_voxels": int(masks.sum(dtype=torch.int64))}
    for approximate in (False, True):
        def call():
            return ctx.contour_trace(masks, a_.size, S, approximate, with_cracks=True)

        for _ in range(2):
            call()
        times = []
        for _ in range(a_.reps):
            ms, (verts, rows, hole, cracks) = event_ms(call)
            times.append(ms)
        key = "approximate" if approximate else "full"
        result[key] = {"call": stats(times, nbytes), "cracks": cracks, "vertices": int(verts.shape[0]), "contours": int(rows.size),
                       "holes": int(hole.sum())}
        ctx.contour_fill(verts, rows, a_.size, S, back)
        result[key]["round_trip_equal"] = bool(torch.equal(back, masks))
        if not approximate:
            ctx.profile_enable(True)
            ctx.profile_read()
            parts = {name: [] for name, _ in STAGES}
            for _ in range(a_.reps):
                call()
                prof = ctx.profile_read()
                for name in parts:
                    parts[name].append(prof[name][1])
            ctx.profile_enable(False)
            result[key]["stages"] = {k: stats(parts[name], nbytes if k.startswith("stream") else None) for name, k in STAGES}

    # the yardstick of the stream passes: a byte kernel over the same bytes
    for _ in range(2):
        ctx.slice_contour(masks, (nx, ny, nz * S), back)
    t = [event_ms(lambda: ctx.slice_contour(masks, (nx, ny, nz * S), back))[0] for _ in range(a_.reps)]
    result["slice_contour"] = stats(t, nbytes)
    stages = result["full"]["stages"]
    result["stream_count_over_slice_contour"] = round(stages["stream_count"]["ms_median"] / result["slice_contour"]["ms_median"], 2)
    result["stream_emit_over_slice_contour"] = round(stages["stream_emit"]["ms_median"] / result["slice_contour"]["ms_median"], 2)
    result["call_over_slice_contour"] = round(result["full"]["call"]["ms_median"] / result["slice_contour"]["ms_median"], 2)

    assert result["full"]["round_trip_equal"], "filling the extracted contours does not give the masks back"
    out_line = json.dumps(result)
    print(out_line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as fh:
            fh.write(out_line + "\n")


if __name__ == "__main__":
    main()
