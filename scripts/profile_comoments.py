#!/usr/bin/env python3
"""Covariance of two fields on segments (mdb_comoments_buckets_dev) by kernel, beside two comparisons made of existing
entry points with the same request on the same resident batches, in one process:
  (a) mdb_moments_buckets_dev(x) + mdb_moments_buckets_dev(y): the two variance states without the covariance;
  (b) mdb_grid_batch_range_dev of x with timestamps + the values-only range grid of y: the floor of the plan a user has
      today (both fields rebuilt in HBM), before any reduction.
Batches: the workload of scripts/profile_moments.py with a second field of the same series - bench.py's synthetic
series (1 ms interval, chunks of 65 536 points; x relative 1 %, y another seed under relative 5 %, so the fields are cut
differently), fitted by compress_chunks_dev, one group per series; and the mixed series of tests/datagen.py (0.1 ms)
lossless for both fields (MacaqueV streams, decoded from the cursor index). Two requests each: about 2 000 buckets over
the data (a screen), and buckets of 7 intervals (many pairs). Each figure: a warm-up call, then --samples samples, each
the mean of --repeats calls between device synchronisations (a call takes 0.3 to 3 ms: 20 of them are a window of tens
of milliseconds); the figure is the median of the samples, given with the smallest and the largest, beside the kernels'
HIP-event times and launches of one more profiled call. Run the script more than once to see the spread between
processes. The claim to test: comoments takes less time than (b). Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_comoments.py [--series N] [--points P] [--repeats R] [--samples S]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import modelardb_rs_amd as mdb  # noqa: E402
import datagen  # noqa: E402
from profile_moments import I64_MAX, I64_MIN, SEED, fitted_batch  # noqa: E402

SAMPLES = 9


def timed(ctx, call, repeats):
    """(median over SAMPLES samples of the mean ms of `repeats` synchronised calls, {kernel: [launches, ms]} of one
    profiled call, [smallest, largest] sample)."""
    call()
    ctx.sync()
    samples = []
    for _ in range(SAMPLES):
        started = time.perf_counter()
        for _ in range(repeats):
            call()
            ctx.sync()
        samples.append((time.perf_counter() - started) / repeats * 1e3)
    ctx.profile_enable(True)
    ctx.profile_reset()
    call()
    ctx.sync()
    kernels = {name: [launches, round(total_ms, 4)] for name, (launches, total_ms) in ctx.profile().items()}
    ctx.profile_enable(False)
    return float(np.median(samples)), kernels, [round(min(samples), 4), round(max(samples), 4)]


def both(first, second):
    def call():
        first()
        second()
    return call


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
    # (y's segments are other rows than x's: its groups for comparison (a))
    y_groups = np.searchsorted(np.flatnonzero(np.diff(np.concatenate([[-1], y.start_time])) < 0), np.arange(len(y)),
                               side="right").astype(np.uint32)
    assert int(y_groups.max()) == n_groups - 1
    dev_y_groups = ctx.upload_array(y_groups)
    try:
        rebuild = timed(ctx, both(
            lambda: ctx.grid_batch_range_dev(dev_x, I64_MIN, I64_MAX, out_ts, out_val, n_points),
            lambda: ctx.grid_batch_range_dev(dev_y, I64_MIN, I64_MAX, None, out_y, n_points)), repeats)
        y_only = timed(ctx, lambda: ctx.grid_batch_range_dev(dev_y, I64_MIN, I64_MAX, None, out_y, n_points), repeats)
        result.update(rebuild_both_ms=round(rebuild[0], 4), rebuild_both_range_ms=rebuild[2], rebuild_kernels=rebuild[1],
                      rebuild_y_values_only_ms=round(y_only[0], 4))
        for label, width in (("screen", (last - first) // 2000 + 1), ("7_intervals", 7 * interval)):
            n_buckets = (last - first) // width + 1
            request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, 0)
            dev_cells = ctx.upload_array(mdb.fresh_comoments_cells((n_groups, n_buckets)))
            cells_x = ctx.upload_array(mdb.fresh_moments_cells((n_groups, n_buckets)))
            cells_y = ctx.upload_array(mdb.fresh_moments_cells((n_groups, n_buckets)))
            comoments = timed(ctx, lambda: ctx._check(ctx.lib.mdb_comoments_buckets_dev(
                ctx.handle, ctypes.byref(dev_x.seg), ctypes.byref(dev_y.seg), ctypes.c_void_p(dev_groups),
                ctypes.byref(request), ctypes.c_void_p(dev_cells))), repeats)
            moments = timed(ctx, both(
                lambda: ctx._check(ctx.lib.mdb_moments_buckets_dev(
                    ctx.handle, ctypes.byref(dev_x.seg), ctypes.c_void_p(dev_groups), ctypes.byref(request),
                    ctypes.c_void_p(cells_x))),
                lambda: ctx._check(ctx.lib.mdb_moments_buckets_dev(
                    ctx.handle, ctypes.byref(dev_y.seg), ctypes.c_void_p(dev_y_groups), ctypes.byref(request),
                    ctypes.c_void_p(cells_y)))), repeats)
            counted = int(ctx.download_array(dev_cells, n_groups * n_buckets, mdb.COMOMENTS_CELL_DTYPE)["count"].sum())
            assert counted == (SAMPLES * repeats + 2) * n_points, (counted, n_points)   # (every call merged the batch once more)
            for pointer in (dev_cells, cells_x, cells_y):
                ctx.dev_free(pointer)
            kernel_ms = sum(ms for _, ms in comoments[1].values())
            partials_ms = comoments[1].get("k_comoments_partials", [0, 0.0])[1]
            result["requests"].append({
                "request": label, "width": width, "n_buckets": n_buckets, "cells": n_groups * n_buckets,
                "comoments_ms": round(comoments[0], 4), "comoments_range_ms": comoments[2],
                "comoments_kernels": comoments[1], "moments_x_plus_y_ms": round(moments[0], 4),
                "moments_range_ms": moments[2], "moments_kernels": moments[1],
                "comoments_over_two_moments": round(comoments[0] / moments[0], 3),
                "comoments_over_rebuild": round(comoments[0] / rebuild[0], 3),
                "below_rebuild": bool(comoments[0] < rebuild[0]),
                "partials_share_of_kernel_time": round(partials_ms / kernel_ms, 3) if kernel_ms else None,
                "comoments_points_per_s": round(n_points / (comoments[0] * 1e-3), 1)})
            spread = lambda figure: f"{figure[0]:9.3f} ms [{figure[2][0]:.3f} .. {figure[2][1]:.3f}]"
            print(f"{name:28s} {label:12s} {n_buckets:9d} buckets  comoments {spread(comoments)}  (a) two moments "
                  f"{spread(moments)}  (b) rebuild of both fields {spread(rebuild)} (y alone {y_only[0]:9.3f})  "
                  f"k_comoments_partials {partials_ms:9.3f} of {kernel_ms:9.3f} ms in kernels  {n_points} points", flush=True)
    finally:
        for pointer in (out_ts, out_val, out_y, dev_groups, dev_y_groups):
            ctx.dev_free(pointer)
        dev_x.free()
        dev_y.free()
    return result


def main():
    global SAMPLES
    parser = argparse.ArgumentParser()
    parser.add_argument("--series", type=int, default=10)
    parser.add_argument("--points", type=int, default=10_000_000)
    parser.add_argument("--mixed-series", type=int, default=16)
    parser.add_argument("--mixed-points", type=int, default=1_000_000)
    parser.add_argument("--repeats", type=int, default=20)
    parser.add_argument("--samples", type=int, default=9)
    parser.add_argument("--skip-mixed", action="store_true")
    a = parser.parse_args()
    SAMPLES = a.samples
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
