#!/usr/bin/env python3
"""Aggregates per date_bin bucket and group (mdb_agg_buckets_dev) against grid() (mdb_grid_batch_dev) of the same
resident batch - grid alone is a lower bound for the reference's plan (GridExec + date_bin + GROUP BY) - on
  * a bench-shaped batch: bench.py's synthetic series (1 ms interval, chunks of 65 536 points, relative 1 %), fitted
    by compress_chunks_dev, --series of --points points (the headline: --series 1000);
  * the mixed series of tests/datagen.py (0.1 ms interval), lossless and relative 1 %.
Bucket widths of 1 000, 60 000 and 3 600 000 sampling intervals, one group per series and one group over all series
(the sort path). Each figure: a warm-up call, then the mean of --repeats calls between device synchronisations, with
the kernels' HIP-event times of one more profiled call. grid() of the bench-shaped batch is timed per fitting group
of series (its output for 10^10 points does not fit HBM twice) and summed. Prints one JSON line at the end.
Usage (on the GPU box): python3 scripts/profile_bucket_aggregates.py [--series N] [--points P] [--repeats R]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import modelardb_rs_amd as mdb  # noqa: E402
from modelardb_rs_amd import _abi  # noqa: E402
import datagen  # noqa: E402

CHUNK_POINTS = 65536
SEED = 0x4D44425F52454631  # bench.py's
MASK = mdb.MDB_AGG_COUNT | mdb.MDB_AGG_MIN | mdb.MDB_AGG_MAX | mdb.MDB_AGG_SUM
WIDTHS = (1_000, 60_000, 3_600_000)  # sampling intervals


def timed(ctx, call, repeats):
    """(mean ms over `repeats` synchronised calls, {kernel: ms} of one profiled call)."""
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
    kernels = {name: round(total_ms, 4) for name, (_, total_ms) in ctx.profile().items()}
    ctx.profile_enable(False)
    return ms, kernels


def grid_ms(ctx, resident, repeats):
    n = ctx.grid_count_dev(resident)
    out_ts, out_val = ctx.dev_alloc(8 * n), ctx.dev_alloc(4 * n)
    try:
        return timed(ctx, lambda: ctx.grid_batch_dev(resident, out_ts, out_val, n), repeats)
    finally:
        ctx.dev_free(out_ts)
        ctx.dev_free(out_val)


def buckets_ms(ctx, resident, span, series_of_segment, interval, width, repeats, per_series):
    """mdb_agg_buckets_dev with device arrays made once (the cells keep folding: the figure is the call's)."""
    first, last = span
    n_buckets = (last - first) // (width * interval) + 1
    n_groups = int(series_of_segment.max()) + 1 if per_series else 1
    groups = ctx.upload_array(series_of_segment.astype(np.uint32)) if per_series else None
    states = ctx.upload_array(mdb.fresh_agg_states(n_groups * n_buckets))
    request = _abi.BucketRequestC(first, width * interval, n_buckets, -(1 << 63), (1 << 63) - 1, n_groups, MASK)

    def call():
        ctx._check(ctx.lib.mdb_agg_buckets_dev(ctx.handle, C.byref(resident.seg), None if groups is None else C.c_void_p(groups),
                                               C.byref(request), C.c_void_p(states)))
    try:
        ms, kernels = timed(ctx, call, repeats)
    finally:
        ctx.dev_free(states)
        if groups is not None:
            ctx.dev_free(groups)
    return {"width_intervals": width, "groups": "per series" if per_series else "one", "cells": n_groups * n_buckets,
            "ms": round(ms, 4), "kernels_ms": kernels}


def measure(ctx, name, batch, series_of_segment, interval, grid, repeats):
    resident = ctx.upload_segments(batch)
    span = (int(batch.start_time.min()), int(batch.end_time.max()))
    if grid is None:
        grid = grid_ms(ctx, resident, repeats)
    runs = []
    for width in WIDTHS:
        for per_series in (True, False):
            run = buckets_ms(ctx, resident, span, series_of_segment, interval, width, repeats, per_series)
            run["x_faster_than_grid"] = round(grid[0] / run["ms"], 2)
            print(f"{name:28s} {len(batch):10d} segments  width {width:9d}  groups {run['groups']:10s} "
                  f"{run['ms']:9.3f} ms  grid {grid[0]:8.3f} ms  x{run['x_faster_than_grid']:6.2f}  {run['kernels_ms']}",
                  flush=True)
            runs.append(run)
    resident.free()
    types = np.bincount(batch.model_type_id.astype(np.int64), minlength=3)
    return {"batch": name, "segments": len(batch), "model_types": types.tolist(),
            "with_residuals": int((batch.residuals.lengths() > 0).sum()), "grid_ms": round(grid[0], 4),
            "grid_kernels_ms": grid[1], "buckets": runs}


def bench_shaped(ctx, a):
    """bench.py's fit, in groups of series; grid() timed per group."""
    eb = mdb.error_bound("relative", 1.0)
    parts, series_ids, grid_total, grid_kernels = [], [], 0.0, {}
    starts = np.arange(0, a.points, CHUNK_POINTS, dtype=np.uint64)
    for first in range(0, a.series, a.group):
        n_series = min(a.group, a.series - first)
        total = n_series * a.points
        values = ctx.dev_alloc(4 * total)
        ctx.synth_values_dev(values, first, n_series, a.points, SEED)
        offsets = (np.arange(n_series, dtype=np.uint64)[:, None] * np.uint64(a.points) + starts[None, :]).reshape(-1)
        offsets = np.concatenate([offsets, np.array([total], dtype=np.uint64)])
        offsets_dev, first_index_dev = ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, n_series))
        fitted = ctx.compress_chunks_dev(0, values, offsets_dev, len(offsets) - 1, eb, 0, 1000, first_index_dev)
        ctx.sync()
        for pointer in (values, offsets_dev, first_index_dev):
            ctx.dev_free(pointer)
        ms, kernels = grid_ms(ctx, fitted, a.repeats)
        grid_total += ms
        for k, v in kernels.items():
            grid_kernels[k] = round(grid_kernels.get(k, 0.0) + v, 4)
        part = fitted.download()
        fitted.free()
        parts.append(part)
        series_ids.append(first + part.chunk_index.astype(np.int64) // len(starts))
    batch = mdb.SegmentBatch.concat(parts)
    return measure(ctx, f"bench {a.series}x{a.points}", batch, np.concatenate(series_ids), 1000,
                   (grid_total, grid_kernels), a.repeats)


def mixed(ctx, a, bound):
    eb = mdb.error_bound("lossless") if bound == "lossless" else mdb.error_bound("relative", 1.0)
    points = a.mixed_points
    host_values = np.concatenate([datagen.mixed_series(points, 1000 + s, (1.0, 1.05) if s % 2 else None)[1]
                                  for s in range(a.mixed_series)])
    values = ctx.upload_array(host_values)
    starts = np.arange(0, points, CHUNK_POINTS, dtype=np.uint64)
    offsets = np.concatenate([s * points + starts for s in range(a.mixed_series)] +
                             [np.array([a.mixed_series * points], dtype=np.uint64)]).astype(np.uint64)
    offsets_dev, first_index_dev = ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, a.mixed_series))
    fitted = ctx.compress_chunks_dev(0, values, offsets_dev, len(offsets) - 1, eb, 0, 100, first_index_dev)
    ctx.sync()
    for pointer in (values, offsets_dev, first_index_dev):
        ctx.dev_free(pointer)
    batch = fitted.download()
    fitted.free()
    series = batch.chunk_index.astype(np.int64) // len(starts)
    return measure(ctx, f"mixed {bound} {a.mixed_series}x{points}", batch, series, 100, None, a.repeats)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--series", type=int, default=100)
    parser.add_argument("--points", type=int, default=10_000_000)
    parser.add_argument("--group", type=int, default=100, help="series per fit (and per timed grid)")
    parser.add_argument("--mixed-series", type=int, default=64)
    parser.add_argument("--mixed-points", type=int, default=1_000_000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--skip-mixed", action="store_true")
    a = parser.parse_args()
    ctx = mdb.Context(0)
    results = [bench_shaped(ctx, a)]
    if not a.skip_mixed:
        results += [mixed(ctx, a, "lossless"), mixed(ctx, a, "1%")]
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
