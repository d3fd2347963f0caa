#!/usr/bin/env python3
"""Aggregates per date_bin bucket and group with a value predicate (mdb_agg_buckets_filter_dev) against the unfiltered
bucket call (mdb_agg_buckets_dev) of the same resident batch and width and - on the mixed series - against the filtered
aggregates of the whole batch (mdb_agg_batch_filter_dev), on
  * a bench-shaped batch: bench.py's synthetic series (1 ms interval, chunks of 65 536 points, relative 1 %), fitted
    by compress_chunks_dev, --series of --points points (the headline: --series 1000);
  * the mixed series of tests/datagen.py (0.1 ms interval), lossless and relative 1 %.
1-minute buckets, one group per series. Selectivities 0, 1, 10, 50 and 100 %: `value >= q` with q the (1 - s) quantile
of a sample of the rebuilt points of the first series (0 %: above every value; 100 %: -inf); "passing" is the share of
the unfiltered call's points that a fresh filtered call counts. Each figure: a warm-up call, then the mean of --repeats
calls between device synchronisations, with the kernels' HIP-event times of one more profiled call. Prints one JSON
line at the end.
Usage (on the GPU box): python3 scripts/profile_bucket_filter.py [--series N] [--points P] [--repeats R]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import modelardb_rs_amd as mdb  # noqa: E402
from modelardb_rs_amd import _abi  # noqa: E402
import datagen  # noqa: E402
from profile_bucket_aggregates import CHUNK_POINTS, MASK, SEED, timed  # noqa: E402

SELECTIVITIES = (0.0, 0.01, 0.10, 0.50, 1.0)
MINUTE_US = 60_000_000
SAMPLE_SERIES = 8
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def thresholds(ctx, batch, series_of_segment):
    """Filters of the five selectivities from a sample of the rebuilt points of the first SAMPLE_SERIES series."""
    resident = ctx.upload_segments(batch.take(np.nonzero(series_of_segment < SAMPLE_SERIES)[0]))
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    out_ts, out_val = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points)
    try:
        ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, out_ts, out_val, n_points)
        step = max(n_points // (1 << 20), 1)
        sample = np.concatenate([ctx.download_array(out_val, min(4096, n_points - k), np.float32, k)
                                 for k in range(0, n_points, step * 4096)])
    finally:
        ctx.dev_free(out_ts)
        ctx.dev_free(out_val)
        resident.free()
    sample = np.sort(sample[np.isfinite(sample)])
    out = []
    for s in SELECTIVITIES:
        if s == 0.0:
            out.append((s, mdb.value_filter(lo=float(sample[-1]) * 2.0 + 1e30)))
        elif s == 1.0:
            out.append((s, mdb.value_filter(lo=-np.inf)))
        else:
            out.append((s, mdb.value_filter(lo=float(sample[int((1.0 - s) * (len(sample) - 1))]))))
    return out


def measure(ctx, name, batch, series_of_segment, repeats, with_batch_filter):
    filters = thresholds(ctx, batch, series_of_segment)
    resident = ctx.upload_segments(batch)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    n_groups = int(series_of_segment.max()) + 1
    n_buckets = (last - first) // MINUTE_US + 1
    n_cells = n_groups * n_buckets
    groups = ctx.upload_array(series_of_segment.astype(np.uint32))
    states = ctx.upload_array(mdb.fresh_agg_states(n_cells))
    request = _abi.BucketRequestC(first, MINUTE_US, n_buckets, I64_MIN, I64_MAX, n_groups, MASK)

    def plain():
        ctx._check(ctx.lib.mdb_agg_buckets_dev(ctx.handle, C.byref(resident.seg), C.c_void_p(groups), C.byref(request),
                                               C.c_void_p(states)))

    def filtered(flt):
        ctx._check(ctx.lib.mdb_agg_buckets_filter_dev(ctx.handle, C.byref(resident.seg), C.c_void_p(groups),
                                                      C.byref(request), C.byref(flt), C.c_void_p(states)))

    def counted(call):
        """The points a call on fresh cells counts (the timed calls keep folding into `states`)."""
        fresh = ctx.upload_array(mdb.fresh_agg_states(n_cells))
        try:
            ctx._check(call(fresh))
            return int(ctx.download_array(fresh, n_cells, mdb.AGG_STATE_DTYPE)["count"].sum())
        finally:
            ctx.dev_free(fresh)

    try:
        plain_ms, plain_kernels = timed(ctx, plain, repeats)
        total = counted(lambda cells: ctx.lib.mdb_agg_buckets_dev(ctx.handle, C.byref(resident.seg), C.c_void_p(groups),
                                                                  C.byref(request), C.c_void_p(cells)))
        print(f"{name:34s} {len(batch):10d} segments  {n_cells:9d} cells  unfiltered {plain_ms:8.3f} ms  {plain_kernels}",
              flush=True)
        runs = []
        for s, flt in filters:
            ms, kernels = timed(ctx, lambda: filtered(flt), repeats)
            passing = counted(lambda cells: ctx.lib.mdb_agg_buckets_filter_dev(
                ctx.handle, C.byref(resident.seg), C.c_void_p(groups), C.byref(request), C.byref(flt),
                C.c_void_p(cells)))
            run = {"selectivity": s, "passing": round(passing / max(total, 1), 5), "ms": round(ms, 4),
                   "x_unfiltered": round(ms / plain_ms, 3), "kernels_ms": kernels}
            if with_batch_filter:
                batch_ms, batch_kernels = timed(ctx, lambda: ctx.agg_filter_dev(resident, flt, MASK), repeats)
                run["batch_filter_ms"], run["batch_filter_kernels_ms"] = round(batch_ms, 4), batch_kernels
            print(f"{name:34s} s={s:5.2f} passing {run['passing']:7.4f}  {ms:8.3f} ms  x{run['x_unfiltered']:6.3f}"
                  f"  {kernels}" + (f"  batch filter {run['batch_filter_ms']:8.3f} ms" if with_batch_filter else ""),
                  flush=True)
            runs.append(run)
    finally:
        ctx.dev_free(states)
        ctx.dev_free(groups)
        resident.free()
    types = np.bincount(batch.model_type_id.astype(np.int64), minlength=3)
    return {"batch": name, "segments": len(batch), "model_types": types.tolist(),
            "with_residuals": int((batch.residuals.lengths() > 0).sum()), "points": total, "cells": n_cells,
            "width_us": MINUTE_US, "unfiltered_ms": round(plain_ms, 4), "unfiltered_kernels_ms": plain_kernels,
            "filtered": runs}


def bench_shaped(ctx, a):
    """bench.py's fit, in groups of series."""
    eb = mdb.error_bound("relative", 1.0)
    parts, series_ids = [], []
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
        part = fitted.download()
        fitted.free()
        parts.append(part)
        series_ids.append(first + part.chunk_index.astype(np.int64) // len(starts))
    return mdb.SegmentBatch.concat(parts), np.concatenate(series_ids)


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
    return batch, batch.chunk_index.astype(np.int64) // len(starts)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--series", type=int, default=100)
    parser.add_argument("--points", type=int, default=10_000_000)
    parser.add_argument("--group", type=int, default=100, help="series per fit")
    parser.add_argument("--mixed-series", type=int, default=64)
    parser.add_argument("--mixed-points", type=int, default=1_000_000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--skip-bench", action="store_true")
    parser.add_argument("--skip-mixed", action="store_true")
    a = parser.parse_args()
    ctx = mdb.Context(0)
    results = []
    if not a.skip_bench:
        batch, series = bench_shaped(ctx, a)
        results.append(measure(ctx, f"bench {a.series}x{a.points}", batch, series, a.repeats, False))
    if not a.skip_mixed:
        for bound in ("lossless", "1%"):
            batch, series = mixed(ctx, a, bound)
            results.append(measure(ctx, f"mixed {bound} {a.mixed_series}x{a.mixed_points}", batch, series, a.repeats,
                                   True))
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
