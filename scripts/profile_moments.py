#!/usr/bin/env python3
"""Variance on segments (mdb_moments_buckets_dev) beside mdb_agg_buckets_dev(COUNT | MIN | MAX | SUM), an operator it
shares its pair machinery with, with the same request on the same resident batch, in one process - and beside the
device half of the only route to the same answer without it: mdb_grid_batch_range_dev (timestamps and values into HBM),
whose 12 B per point would then have to cross PCIe and be reduced on the host.
Batches: bench.py's synthetic series (1 ms interval, chunks of 65 536 points, relative 1 %: about 99.6 % Swing on
regular timestamps), fitted by compress_chunks_dev, one group per series; and the mixed series of tests/datagen.py
(0.1 ms) lossless (MacaqueV streams, decoded from the cursor index). Two requests each: about 2 000 buckets over the
data (a screen), and buckets of 7 intervals (many pairs). Each figure: a warm-up call, then the mean of --repeats calls
between device synchronisations, with the kernels' HIP-event times and launches of one more profiled call.
The claim to confirm: moments takes less time than the grid call alone (32 B per pair written, not 12 B per point).
Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_moments.py [--series N] [--points P] [--repeats R]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import modelardb_rs_amd as mdb  # noqa: E402
import datagen  # noqa: E402

CHUNK_POINTS = 65536
SEED = 0x4D44425F52454631  # bench.py's
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ALL = mdb.MDB_AGG_COUNT | mdb.MDB_AGG_MIN | mdb.MDB_AGG_MAX | mdb.MDB_AGG_SUM


def timed(ctx, call, repeats):
    """(mean ms over `repeats` synchronised calls, {kernel: [launches, ms]} of one profiled call)."""
    call()
    ctx.sync()
    started = time.perf_counter()
    for _ in range(repeats):
        call()
        ctx.sync()
    ms = (time.perf_counter() - started) / repeats * 1e3
    ctx.profile_enable(True)
    ctx.profile_reset()
    call()
    ctx.sync()
    kernels = {name: [launches, round(total_ms, 4)] for name, (launches, total_ms) in ctx.profile().items()}
    ctx.profile_enable(False)
    return ms, kernels


def measure(ctx, name, batch, groups, n_groups, interval, repeats):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    result = {"batch": name, "segments": len(batch), "points": n_points, "groups": n_groups,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist(), "requests": []}
    out_ts, out_val = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points)
    dev_groups = ctx.upload_array(groups)
    try:
        rebuild = timed(ctx, lambda: ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, out_ts, out_val, n_points), repeats)
        result.update(rebuild_points_ms=round(rebuild[0], 4), rebuild_kernels=rebuild[1])
        for label, width in (("screen", (last - first) // 2000 + 1), ("7_intervals", 7 * interval)):
            n_buckets = (last - first) // width + 1
            request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, 0)
            agg_request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, ALL)
            dev_cells = ctx.upload_array(mdb.fresh_moments_cells((n_groups, n_buckets)))
            dev_states = ctx.upload_array(mdb.fresh_agg_states((n_groups, n_buckets)))
            moments = timed(ctx, lambda: ctx._check(ctx.lib.mdb_moments_buckets_dev(
                ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(request),
                ctypes.c_void_p(dev_cells))), repeats)
            agg = timed(ctx, lambda: ctx._check(ctx.lib.mdb_agg_buckets_dev(
                ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(agg_request),
                ctypes.c_void_p(dev_states))), repeats)
            counted = int(ctx.download_array(dev_cells, n_groups * n_buckets, mdb.MOMENTS_CELL_DTYPE)["count"].sum())
            assert counted == (repeats + 2) * n_points, (counted, n_points)   # (every call merged the batch once more)
            ctx.dev_free(dev_cells)
            ctx.dev_free(dev_states)
            kernel_ms = sum(ms for _, ms in moments[1].values())
            partials_ms = moments[1].get("k_moments_partials", [0, 0.0])[1]
            result["requests"].append({
                "request": label, "width": width, "n_buckets": n_buckets, "cells": n_groups * n_buckets,
                "moments_ms": round(moments[0], 4), "moments_kernels": moments[1], "agg_buckets_ms": round(agg[0], 4),
                "agg_kernels": agg[1], "moments_over_agg": round(moments[0] / agg[0], 3),
                "moments_over_rebuild": round(moments[0] / rebuild[0], 3),
                "below_rebuild": bool(moments[0] < rebuild[0]),
                "partials_share_of_kernel_time": round(partials_ms / kernel_ms, 3) if kernel_ms else None,
                "moments_points_per_s": round(n_points / (moments[0] * 1e-3), 1)})
            print(f"{name:28s} {label:12s} {n_buckets:9d} buckets  moments {moments[0]:9.3f} ms  agg_buckets {agg[0]:9.3f} ms  "
                  f"rebuild of the points {rebuild[0]:9.3f} ms  k_moments_partials {partials_ms:9.3f} of {kernel_ms:9.3f} ms in kernels  "
                  f"{n_points} points", flush=True)
    finally:
        for pointer in (out_ts, out_val, dev_groups):
            ctx.dev_free(pointer)
        resident.free()
    return result


def fitted_batch(ctx, values, n_series, points, eb, interval):
    """(batch, the series of every segment row)"""
    starts = np.arange(0, points, CHUNK_POINTS, dtype=np.uint64)
    offsets = (np.arange(n_series, dtype=np.uint64)[:, None] * np.uint64(points) + starts[None, :]).reshape(-1)
    offsets = np.concatenate([offsets, np.array([n_series * points], dtype=np.uint64)])
    offsets_dev, first_index_dev = ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, n_series))
    fitted = ctx.compress_chunks_dev(0, values, offsets_dev, len(offsets) - 1, eb, 0, interval, first_index_dev)
    ctx.sync()
    for pointer in (values, offsets_dev, first_index_dev):
        ctx.dev_free(pointer)
    batch = fitted.download()
    fitted.free()
    if batch.chunk_index is not None:
        groups = (batch.chunk_index.astype(np.int64) // len(starts)).astype(np.uint32)
    else:  # (rows are in series order, and every series begins at the same timestamp)
        groups = (np.cumsum(batch.start_time == batch.start_time.min()) - 1).astype(np.uint32)
    assert int(groups.max()) == n_series - 1 and (np.diff(groups.astype(np.int64)) >= 0).all()
    return batch, groups


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--series", type=int, default=10)
    parser.add_argument("--points", type=int, default=10_000_000)
    parser.add_argument("--mixed-series", type=int, default=16)
    parser.add_argument("--mixed-points", type=int, default=1_000_000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--skip-mixed", action="store_true")
    a = parser.parse_args()
    ctx = mdb.Context(0)
    values = ctx.dev_alloc(4 * a.series * a.points)
    ctx.synth_values_dev(values, 0, a.series, a.points, SEED)
    batch, groups = fitted_batch(ctx, values, a.series, a.points, mdb.error_bound("relative", 1.0), 1000)
    results = [measure(ctx, f"bench {a.series}x{a.points}", batch, groups, a.series, 1000, a.repeats)]
    if not a.skip_mixed:
        host_values = np.concatenate([datagen.mixed_series(a.mixed_points, 1000 + s, (1.0, 1.05) if s % 2 else None)[1]
                                      for s in range(a.mixed_series)])
        batch, groups = fitted_batch(ctx, ctx.upload_array(host_values), a.mixed_series, a.mixed_points,
                                     mdb.error_bound("lossless"), 100)
        results.append(measure(ctx, f"mixed lossless {a.mixed_series}x{a.mixed_points}", batch, groups, a.mixed_series, 100,
                               a.repeats))
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
