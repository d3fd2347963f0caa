#!/usr/bin/env python3
"""The moments of one field per value cell of another (mdb_binned_buckets_dev) by kernel, beside two comparisons with
the same request on the same resident batches, in one process:
  (a) mdb_comoments_buckets_dev(x, y): the same pairs grouped by time only;
  (b) mdb_grid_batch_range_dev of x with timestamps + the values-only range grid of y: the floor of the plan a caller
      has today (both fields rebuilt in HBM), before any binning.
Batches: those of scripts/profile_comoments.py - bench.py's synthetic series (1 ms interval, chunks of 65 536 points; x
relative 1 %, y another seed under relative 5 %), and the mixed series of tests/datagen.py (0.1 ms) lossless for both
fields. Per batch 16 and 1 024 quantile edges of the x values (taken from the range grid of x), each for one bucket
over the data and for about 2 000 buckets. The number of runs of a call - maximal stretches of consecutive pairs of one
x segment inside one bucket and one cell - is counted here, on the host, from the grid of x, the segments' row counts
and the buckets. Each figure: a warm-up call, then --samples samples, each the mean of --repeats calls between device
synchronisations; the figure is the median of the samples, given with the smallest and the largest, beside the kernels'
HIP-event times and launches of one more profiled call. The claim to test: binned takes less time than (b). Prints one
JSON line.
Usage (on the GPU box): python3 scripts/profile_binned.py [--series N] [--points P] [--repeats R] [--samples S]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import modelardb_rs_amd as mdb  # noqa: E402
import datagen  # noqa: E402
import profile_comoments  # noqa: E402
from profile_comoments import both, timed  # noqa: E402
from profile_moments import I64_MAX, I64_MIN, SEED, fitted_batch  # noqa: E402


def count_runs(cells, timestamps, segment_first_rows, origin, width):
    """The runs of a call from the value cell and the timestamp of every row of x and the first row of every segment."""
    new_run = np.zeros(len(cells), dtype=bool)
    new_run[segment_first_rows] = True
    new_run[1:] |= cells[1:] != cells[:-1]
    buckets = (timestamps - origin) // width
    new_run[1:] |= buckets[1:] != buckets[:-1]
    return int(new_run.sum())


def measure(ctx, name, x, y, groups, n_groups, interval, repeats):
    dev_x, dev_y = ctx.upload_segments(x), ctx.upload_segments(y)
    n_points = ctx.grid_count_range_dev(dev_x, I64_MIN, I64_MAX)
    assert n_points == ctx.grid_count_range_dev(dev_y, I64_MIN, I64_MAX)
    first, last = int(x.start_time.min()), int(x.end_time.max())
    types = lambda batch: np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist()
    result = {"batch": name, "segments_x": len(x), "segments_y": len(y), "points": n_points, "groups": n_groups,
              "model_types_x": types(x), "model_types_y": types(y), "requests": []}
    out_ts, out_val, out_y = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points), ctx.dev_alloc(4 * n_points)
    dev_groups = ctx.upload_array(groups)
    try:
        rebuild = timed(ctx, both(
            lambda: ctx.grid_batch_range_dev(dev_x, I64_MIN, I64_MAX, out_ts, out_val, n_points),
            lambda: ctx.grid_batch_range_dev(dev_y, I64_MIN, I64_MAX, None, out_y, n_points)), repeats)
        result.update(rebuild_both_ms=round(rebuild[0], 4), rebuild_both_range_ms=rebuild[2], rebuild_kernels=rebuild[1])
        x_values = ctx.download_array(out_val, n_points, np.float32)
        x_times = ctx.download_array(out_ts, n_points, np.int64)
        rows = (x.end_time - x.start_time) // interval + 1   # (regular timestamps)
        assert int(rows.sum()) == n_points
        segment_first_rows = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64)
        for n_edges in (16, 1024):
            edges = np.unique(np.quantile(x_values[::max(1, n_points // 2_000_000)].astype(np.float64),
                                          np.linspace(0.0, 1.0, n_edges + 2)[1:-1]).astype(np.float32))
            cells = np.searchsorted(edges, x_values, side="right").astype(np.int16)
            n_cells = len(edges) + 1
            for label, width in (("one_bucket", last - first + 1), ("screen", (last - first) // 2000 + 1)):
                n_buckets = (last - first) // width + 1
                request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, 0)
                dev_cells = ctx.upload_array(mdb.fresh_moments_cells((n_groups, n_buckets, n_cells)))
                dev_pairs = ctx.upload_array(mdb.fresh_comoments_cells((n_groups, n_buckets)))
                binned = timed(ctx, lambda: ctx._check(ctx.lib.mdb_binned_buckets_dev(
                    ctx.handle, ctypes.byref(dev_x.seg), ctypes.byref(dev_y.seg), ctypes.c_void_p(dev_groups),
                    ctypes.byref(request), edges.ctypes.data_as(ctypes.c_void_p), len(edges), ctypes.c_void_p(dev_cells))),
                    repeats)
                comoments = timed(ctx, lambda: ctx._check(ctx.lib.mdb_comoments_buckets_dev(
                    ctx.handle, ctypes.byref(dev_x.seg), ctypes.byref(dev_y.seg), ctypes.c_void_p(dev_groups),
                    ctypes.byref(request), ctypes.c_void_p(dev_pairs))), repeats)
                counted = int(ctx.download_array(dev_cells, n_groups * n_buckets * n_cells, mdb.MOMENTS_CELL_DTYPE)["count"].sum())
                calls = profile_comoments.SAMPLES * repeats + 2
                assert counted == calls * n_points, (counted, n_points)   # (every call merged the batch once more)
                for pointer in (dev_cells, dev_pairs):
                    ctx.dev_free(pointer)
                runs = count_runs(cells, x_times, segment_first_rows, first, width)
                kernel_ms = sum(ms for _, ms in binned[1].values())
                partials_ms = binned[1].get("k_binned_partials", [0, 0.0])[1]
                count_ms = binned[1].get("k_binned_count", [0, 0.0])[1]
                result["requests"].append({
                    "request": label, "edges": len(edges), "width": width, "n_buckets": n_buckets,
                    "cells": n_groups * n_buckets * n_cells, "runs": runs, "points_per_run": round(n_points / runs, 2),
                    "binned_ms": round(binned[0], 4), "binned_range_ms": binned[2], "binned_kernels": binned[1],
                    "comoments_ms": round(comoments[0], 4), "comoments_range_ms": comoments[2],
                    "binned_over_comoments": round(binned[0] / comoments[0], 3),
                    "binned_over_rebuild": round(binned[0] / rebuild[0], 3), "below_rebuild": bool(binned[0] < rebuild[0]),
                    "partials_share_of_kernel_time": round(partials_ms / kernel_ms, 3) if kernel_ms else None,
                    "binned_points_per_s": round(n_points / (binned[0] * 1e-3), 1)})
                spread = lambda figure: f"{figure[0]:9.3f} ms [{figure[2][0]:.3f} .. {figure[2][1]:.3f}]"
                print(f"{name:28s} {len(edges):5d} edges {label:10s} {n_buckets:6d} buckets {runs:10d} runs  binned "
                      f"{spread(binned)}  (a) comoments {spread(comoments)}  (b) rebuild of both fields {spread(rebuild)}  "
                      f"k_binned_count {count_ms:8.3f} k_binned_partials {partials_ms:8.3f} of {kernel_ms:8.3f} ms in kernels  "
                      f"{n_points} points", flush=True)
    finally:
        for pointer in (out_ts, out_val, out_y, dev_groups):
            ctx.dev_free(pointer)
        dev_x.free()
        dev_y.free()
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--series", type=int, default=10)
    parser.add_argument("--points", type=int, default=10_000_000)
    parser.add_argument("--mixed-series", type=int, default=16)
    parser.add_argument("--mixed-points", type=int, default=1_000_000)
    parser.add_argument("--repeats", type=int, default=10)
    parser.add_argument("--samples", type=int, default=5)
    parser.add_argument("--skip-mixed", action="store_true")
    a = parser.parse_args()
    profile_comoments.SAMPLES = a.samples
    ctx = mdb.Context(0)
    fields = []
    for seed, eb in ((SEED, mdb.error_bound("relative", 1.0)), (SEED ^ 0x5A5A5A5A, mdb.error_bound("relative", 5.0))):
        values = ctx.dev_alloc(4 * a.series * a.points)
        ctx.synth_values_dev(values, 0, a.series, a.points, seed)
        fields.append(fitted_batch(ctx, values, a.series, a.points, eb, 1000))
    results = [measure(ctx, f"bench {a.series}x{a.points}", fields[0][0], fields[1][0], fields[0][1], a.series, 1000, a.repeats)]
    if not a.skip_mixed:
        fields = []
        for base in (1000, 3000):
            host_values = np.concatenate([datagen.mixed_series(a.mixed_points, base + s, (1.0, 1.05) if s % 2 else None)[1]
                                          for s in range(a.mixed_series)])
            fields.append(fitted_batch(ctx, ctx.upload_array(host_values), a.mixed_series, a.mixed_points,
                                       mdb.error_bound("lossless"), 100))
        results.append(measure(ctx, f"mixed lossless {a.mixed_series}x{a.mixed_points}", fields[0][0], fields[1][0],
                               fields[0][1], a.mixed_series, 100, a.repeats))
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
