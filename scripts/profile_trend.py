#!/usr/bin/env python3
"""The linear trend over time on segments (mdb_trend_buckets_dev) beside entry points this change does not touch, with
the same request on the same resident batch, in one process: (a) mdb_moments_buckets_dev - the same walk with two sums in
place of five; (b) mdb_grid_batch_range_dev with timestamps - the floor of today's plan (GridExec -> AggregateExec)
before any reduction; and, for the kernel comparison, (c) mdb_comoments_buckets_dev(x, x), the same five sums with a y
column read per point.
Batches: those of scripts/profile_moments.py - bench.py's synthetic series (1 ms interval, chunks of 65 536 points,
relative 1 %: almost all Swing on regular timestamps), one group per series; and the mixed series of tests/datagen.py
(0.1 ms) lossless (MacaqueV streams, decoded from the cursor index). Two requests each: about 2 000 buckets over the
data (a screen), and buckets of 7 intervals (many pairs). Each figure: a warm-up call, then the median of --samples
samples, a sample the mean of --repeats calls between device synchronisations (wall time, host side included), with the
smallest and the largest sample, beside the kernels' HIP-event times and launches of one more profiled call. Run the
script more than once to see the spread between processes. Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_trend.py [--series N] [--points P] [--repeats R] [--samples S]"""
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
from profile_moments import SEED, fitted_batch  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
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
        result.update(rebuild_points_ms=round(rebuild[0], 4), rebuild_spread=rebuild[2], rebuild_kernels=rebuild[1])
        for label, width in (("screen", (last - first) // 2000 + 1), ("7_intervals", 7 * interval)):
            n_buckets = (last - first) // width + 1
            request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, 0)
            dev_cells = ctx.upload_array(mdb.fresh_comoments_cells((n_groups, n_buckets)))
            dev_pairs = ctx.upload_array(mdb.fresh_comoments_cells((n_groups, n_buckets)))
            dev_moments = ctx.upload_array(mdb.fresh_moments_cells((n_groups, n_buckets)))
            trend = timed(ctx, lambda: ctx._check(ctx.lib.mdb_trend_buckets_dev(
                ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(request),
                ctypes.c_void_p(dev_cells))), repeats)
            moments = timed(ctx, lambda: ctx._check(ctx.lib.mdb_moments_buckets_dev(
                ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(request),
                ctypes.c_void_p(dev_moments))), repeats)
            pairs = timed(ctx, lambda: ctx._check(ctx.lib.mdb_comoments_buckets_dev(
                ctx.handle, ctypes.byref(resident.seg), ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups),
                ctypes.byref(request), ctypes.c_void_p(dev_pairs))), repeats)
            counted = int(ctx.download_array(dev_cells, n_groups * n_buckets, mdb.COMOMENTS_CELL_DTYPE)["count"].sum())
            assert counted == (SAMPLES * repeats + 2) * n_points, (counted, n_points)   # (every call merged the batch once more)
            for pointer in (dev_cells, dev_pairs, dev_moments):
                ctx.dev_free(pointer)
            kernel_ms = sum(ms for _, ms in trend[1].values())
            partials = {kernel: run[1].get(kernel, [0, 0.0])[1]
                        for kernel, run in (("k_trend_partials", trend), ("k_moments_partials", moments),
                                            ("k_comoments_partials", pairs))}
            result["requests"].append({
                "request": label, "width": width, "n_buckets": n_buckets, "cells": n_groups * n_buckets,
                "trend_ms": round(trend[0], 4), "trend_spread": trend[2], "trend_kernels": trend[1],
                "moments_ms": round(moments[0], 4), "moments_spread": moments[2], "moments_kernels": moments[1],
                "comoments_xx_ms": round(pairs[0], 4), "comoments_xx_spread": pairs[2], "comoments_xx_kernels": pairs[1],
                "trend_over_moments": round(trend[0] / moments[0], 3), "trend_over_rebuild": round(trend[0] / rebuild[0], 3),
                "trend_over_comoments_xx": round(trend[0] / pairs[0], 3), "partials_ms": partials,
                "partials_share_of_kernel_time": round(partials["k_trend_partials"] / kernel_ms, 3) if kernel_ms else None,
                "trend_points_per_s": round(n_points / (trend[0] * 1e-3), 1)})
            print(f"{name:28s} {label:12s} {n_buckets:9d} buckets  trend {trend[0]:8.3f} ms {trend[2]}  (a) moments "
                  f"{moments[0]:8.3f} ms {moments[2]}  (b) rebuild {rebuild[0]:8.3f} ms {rebuild[2]}  (c) comoments(x, x) "
                  f"{pairs[0]:8.3f} ms  partials: trend {partials['k_trend_partials']:.3f} moments "
                  f"{partials['k_moments_partials']:.3f} comoments {partials['k_comoments_partials']:.3f} ms; trend kernels "
                  f"{kernel_ms:.3f} ms  {n_points} points", flush=True)
    finally:
        for pointer in (out_ts, out_val, dev_groups):
            ctx.dev_free(pointer)
        resident.free()
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
