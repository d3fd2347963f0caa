#!/usr/bin/env python3
"""Histograms and exact quantiles per date_bin bucket and group (mdb_hist_buckets_dev at 64 edges, mdb_quantile_buckets_dev
for the median and for p50 / p95 / p99) beside the routes to the same answer without them, with the same request on the
same resident batch, in one process:
  - mdb_grid_batch_range_dev, the device half of rebuild-then-bin (12 B per point would then cross PCIe);
  - for the request of about 2 000 buckets, one mdb_hist_batch_dev / mdb_quantile_batch_dev call per bucket;
  - mdb_agg_buckets_dev(COUNT | MIN | MAX | SUM), the sibling operator.
Batches and requests: those of scripts/profile_moments.py - bench.py's synthetic series (1 ms interval, chunks of 65 536
points, relative 1 %: about 99.6 % Swing on regular timestamps), one group per series, and the mixed series of
tests/datagen.py (0.1 ms) lossless (MacaqueV streams); about 2 000 buckets over the data, and buckets of 7 intervals.
Each figure: a warm-up call, then the mean of --repeats calls between device synchronisations (the per-bucket loops: one
warm loop, then one timed loop), with the kernels' HIP-event times and launches of one more profiled call. A request whose
counters the device refuses is reported as refused: that is the documented error.
Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_hist_buckets.py [--series N] [--points P] [--repeats R]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import modelardb_rs_amd as mdb  # noqa: E402
import datagen  # noqa: E402
from profile_moments import ALL, I64_MAX, I64_MIN, SEED, fitted_batch, timed  # noqa: E402

N_EDGES = 64
QUANTILES = {"median": [0.5], "p50_p95_p99": [0.5, 0.95, 0.99]}


def kernel_share(kernels, name):
    total = sum(ms for _, ms in kernels.values())
    return round(kernels.get(name, [0, 0.0])[1] / total, 3) if total else None


def measure(ctx, name, batch, groups, n_groups, interval, repeats):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    lo, hi = float(np.nanmin(batch.min_value)), float(np.nanmax(batch.max_value))
    edges = np.linspace(lo, hi, N_EDGES + 2)[1:-1].astype(np.float32)
    result = {"batch": name, "segments": len(batch), "points": n_points, "groups": n_groups, "edges": len(edges),
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist(), "requests": []}
    out_ts, out_val = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points)
    dev_groups = ctx.upload_array(groups)
    seg, group_pointer = ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups)
    edge_pointer = edges.ctypes.data_as(ctypes.c_void_p)
    try:
        rebuild = timed(ctx, lambda: ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, out_ts, out_val, n_points), repeats)
        result.update(rebuild_points_ms=round(rebuild[0], 4), rebuild_kernels=rebuild[1])
        for label, width in (("screen", (last - first) // 2000 + 1), ("7_intervals", 7 * interval)):
            n_buckets = (last - first) // width + 1
            request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, 0)
            agg_request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, ALL)
            row = {"request": label, "width": width, "n_buckets": n_buckets, "cells": n_groups * n_buckets,
                   "hist_counter_bytes": n_groups * n_buckets * (len(edges) + 1) * 8}
            dev_states = ctx.upload_array(mdb.fresh_agg_states((n_groups, n_buckets)))
            agg = timed(ctx, lambda: ctx._check(ctx.lib.mdb_agg_buckets_dev(ctx.handle, seg, group_pointer, ctypes.byref(agg_request),
                                                                            ctypes.c_void_p(dev_states))), repeats)
            ctx.dev_free(dev_states)
            row.update(agg_buckets_ms=round(agg[0], 4), agg_kernels=agg[1])
            # the histogram
            try:
                counts = torch.zeros(row["hist_counter_bytes"] // 8, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                hist = timed(ctx, lambda: ctx._check(ctx.lib.mdb_hist_buckets_dev(
                    ctx.handle, seg, group_pointer, ctypes.byref(request), edge_pointer, len(edges),
                    ctypes.c_void_p(counts.data_ptr()))), repeats)
                counted = int(counts.sum().item())
                del counts
                assert counted == (repeats + 2) * n_points, (counted, n_points)   # (every call added the batch once more)
                row.update(hist_ms=round(hist[0], 4), hist_kernels=hist[1], hist_over_rebuild=round(hist[0] / rebuild[0], 3),
                           hist_over_agg=round(hist[0] / agg[0], 3),
                           hist_counting_share_of_kernel_time=kernel_share(hist[1], "k_hist_buckets"),
                           hist_points_per_s=round(n_points / (hist[0] * 1e-3), 1))
            except (mdb.HipError, torch.OutOfMemoryError) as refused:
                row.update(hist_ms=None, hist_refused=str(refused)[:200])
            # the quantiles
            for q_name, q in QUANTILES.items():
                q_array = np.array(q, dtype=np.float64)
                lo_out = np.zeros(n_groups * n_buckets * len(q), dtype=np.float32)
                hi_out, counted = lo_out.copy(), np.zeros(n_groups * n_buckets, dtype=np.uint64)
                row[q_name + "_counter_bytes"] = n_groups * n_buckets * 2 * len(q) * 256 * 8
                try:
                    quantile = timed(ctx, lambda: ctx._check(ctx.lib.mdb_quantile_buckets_dev(
                        ctx.handle, seg, group_pointer, ctypes.byref(request), q_array.ctypes.data, len(q), lo_out.ctypes.data,
                        hi_out.ctypes.data, counted.ctypes.data)), repeats)
                    assert int(counted.sum()) == n_points, (int(counted.sum()), n_points)
                    row.update({q_name + "_ms": round(quantile[0], 4), q_name + "_kernels": quantile[1],
                                q_name + "_over_rebuild": round(quantile[0] / rebuild[0], 3),
                                q_name + "_over_agg": round(quantile[0] / agg[0], 3),
                                q_name + "_counting_share_of_kernel_time": kernel_share(quantile[1], "k_hist_buckets_window")})
                except mdb.HipError as refused:
                    row.update({q_name + "_ms": None, q_name + "_refused": str(refused)})
            # one call per bucket, as before this operator: the screen request only
            if label == "screen":
                hist_request = [mdb._abi.HistRequestC(first + b * width, first + (b + 1) * width - 1, len(edges), n_groups, 0, 0)
                                for b in range(n_buckets)]
                dev_one = ctx.upload_array(np.zeros((n_groups, len(edges) + 1), dtype=np.uint64))
                one_lo, one_hi, one_n = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32), ctypes.c_uint64()

                def hist_loop():
                    for r in hist_request:
                        ctx._check(ctx.lib.mdb_hist_batch_dev(ctx.handle, seg, group_pointer, ctypes.byref(r), edge_pointer,
                                                              ctypes.c_void_p(dev_one)))

                def quantile_loop(q_array):
                    # (mdb_quantile_batch_dev has no groups: one call per bucket answers the ungrouped question only)
                    for r in hist_request:
                        ctx._check(ctx.lib.mdb_quantile_batch_dev(ctx.handle, seg, r.t_lo, r.t_hi, q_array.ctypes.data, len(q_array),
                                                                  one_lo.ctypes.data, one_hi.ctypes.data, ctypes.byref(one_n)))

                loops = {"hist_per_bucket_calls_ms": hist_loop}
                for q_name, q in QUANTILES.items():
                    loops[q_name + "_per_bucket_calls_ms"] = (lambda q_array=np.array(q, dtype=np.float64): quantile_loop(q_array))
                for key, loop in loops.items():
                    loop()
                    ctx.sync()
                    started = time.perf_counter()
                    loop()
                    ctx.sync()
                    row[key] = round((time.perf_counter() - started) * 1e3, 3)
                ctx.dev_free(dev_one)
                if row.get("hist_ms"):
                    row["hist_per_bucket_calls_over_hist"] = round(row["hist_per_bucket_calls_ms"] / row["hist_ms"], 1)
                for q_name in QUANTILES:
                    if row.get(q_name + "_ms"):
                        row[q_name + "_per_bucket_calls_over_it"] = round(row[q_name + "_per_bucket_calls_ms"] / row[q_name + "_ms"], 1)
            result["requests"].append(row)
            print(f"{name:28s} {label:12s} {n_buckets:9d} buckets  hist {row.get('hist_ms')} ms  median {row.get('median_ms')} ms  "
                  f"p50/p95/p99 {row.get('p50_p95_p99_ms')} ms  agg_buckets {agg[0]:.3f} ms  rebuild {rebuild[0]:.3f} ms  "
                  f"per-bucket calls: hist {row.get('hist_per_bucket_calls_ms')} ms, median {row.get('median_per_bucket_calls_ms')} ms  "
                  f"{n_points} points", flush=True)
    finally:
        for pointer in (out_ts, out_val, dev_groups):
            ctx.dev_free(pointer)
        resident.free()
    return result


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
