#!/usr/bin/env python3
"""Time-weighted averages and integrals on segments (mdb_integral_buckets_dev, LINEAR and STEP) beside two per-bucket
operators this change does not touch, with the same bucket request on the same resident batch, in one process:
(a) mdb_agg_buckets_dev with SUM - the same closed forms per (segment, bucket) pair, a 24-byte partial; (b)
mdb_trend_buckets_dev - the walk that does strictly more per Swing point.
Batches: those of scripts/profile_moments.py - bench.py's synthetic series (1 ms interval, chunks of 65 536 points,
relative 1 %: almost all Swing on regular timestamps), one group per series; and the mixed series of tests/datagen.py
(0.1 ms) lossless (MacaqueV streams: one lane per stream here, the cursor index for the other two). Two requests each:
about 2 000 buckets over the data (a screen), and buckets of 7 intervals (many pairs). max_gap is the sampling
interval. Each figure: a warm-up call, then the median of --samples samples, a sample the mean of --repeats calls
between device synchronisations (wall time, host side included), with the smallest and the largest sample, beside the
kernels' HIP-event times and launches of one more profiled call. Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_integral.py [--series N] [--points P] [--repeats R] [--samples S]"""
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
import profile_trend  # noqa: E402
from profile_moments import SEED, fitted_batch  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def measure(ctx, name, batch, groups, n_groups, interval, repeats):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    result = {"batch": name, "segments": len(batch), "points": n_points, "groups": n_groups,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist(), "requests": []}
    dev_groups = ctx.upload_array(groups)
    try:
        for label, width in (("screen", (last - first) // 2000 + 1), ("7_intervals", 7 * interval)):
            n_buckets = (last - first) // width + 1
            request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, 0)
            sums = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, mdb.MDB_AGG_SUM)
            runs = {}
            for method_name, method in (("linear", mdb.MDB_INTEGRAL_LINEAR), ("step", mdb.MDB_INTEGRAL_STEP)):
                integral_request = ctx._integral_request(first, width, n_buckets, n_groups, method, interval)
                dev_cells = ctx.upload_array(mdb.fresh_integral_cells((n_groups, n_buckets)))
                runs[method_name] = profile_trend.timed(ctx, lambda: ctx._check(ctx.lib.mdb_integral_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(integral_request),
                    ctypes.c_void_p(dev_cells))), repeats)
                cells = ctx.download_array(dev_cells, n_groups * n_buckets, mdb.INTEGRAL_CELL_DTYPE)
                # (every call merged the batch once more: each series' linked time is its points less one, times the interval)
                calls = profile_trend.SAMPLES * repeats + 2
                assert int(cells["duration"].sum()) == calls * (n_points - n_groups) * interval, name
                ctx.dev_free(dev_cells)
            dev_states = ctx.upload_array(mdb.fresh_agg_states((n_groups, n_buckets)))
            dev_trend = ctx.upload_array(mdb.fresh_comoments_cells((n_groups, n_buckets)))
            runs["sum"] = profile_trend.timed(ctx, lambda: ctx._check(ctx.lib.mdb_agg_buckets_dev(
                ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(sums),
                ctypes.c_void_p(dev_states))), repeats)
            runs["trend"] = profile_trend.timed(ctx, lambda: ctx._check(ctx.lib.mdb_trend_buckets_dev(
                ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(request),
                ctypes.c_void_p(dev_trend))), repeats)
            for pointer in (dev_states, dev_trend):
                ctx.dev_free(pointer)
            entry = {"request": label, "width": width, "n_buckets": n_buckets, "cells": n_groups * n_buckets}
            for key, run in runs.items():
                entry.update({f"{key}_ms": round(run[0], 4), f"{key}_spread": run[2], f"{key}_kernels": run[1],
                              f"{key}_kernel_ms": round(sum(ms for _, ms in run[1].values()), 4)})
            entry.update(linear_over_sum=round(runs["linear"][0] / runs["sum"][0], 3),
                         linear_over_trend=round(runs["linear"][0] / runs["trend"][0], 3),
                         step_over_sum=round(runs["step"][0] / runs["sum"][0], 3),
                         linear_points_per_s=round(n_points / (runs["linear"][0] * 1e-3), 1))
            result["requests"].append(entry)
            print(f"{name:28s} {label:12s} {n_buckets:9d} buckets  integral linear {runs['linear'][0]:8.3f} ms "
                  f"{runs['linear'][2]}  step {runs['step'][0]:8.3f} ms {runs['step'][2]}  (a) SUM {runs['sum'][0]:8.3f} ms "
                  f"{runs['sum'][2]}  (b) trend {runs['trend'][0]:8.3f} ms {runs['trend'][2]}  kernels: linear "
                  f"{entry['linear_kernel_ms']:.3f} step {entry['step_kernel_ms']:.3f} SUM {entry['sum_kernel_ms']:.3f} trend "
                  f"{entry['trend_kernel_ms']:.3f} ms  {n_points} points", flush=True)
    finally:
        ctx.dev_free(dev_groups)
        resident.free()
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--series", type=int, default=10)
    parser.add_argument("--points", type=int, default=10_000_000)
    parser.add_argument("--mixed-series", type=int, default=16)
    parser.add_argument("--mixed-points", type=int, default=1_000_000)
    parser.add_argument("--repeats", type=int, default=20)
    parser.add_argument("--samples", type=int, default=9)
    parser.add_argument("--skip-mixed", action="store_true")
    a = parser.parse_args()
    profile_trend.SAMPLES = a.samples
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
