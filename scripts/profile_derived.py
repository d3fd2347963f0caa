#!/usr/bin/env python3
"""A derived field of two fields per bucket (mdb_derived_buckets_dev with PRODUCT) by kernel, and the generated column
(mdb_derived_values_dev), beside two comparisons with the same request on the same resident batches, in one process:
  (a) mdb_comoments_buckets_dev: the nearest operator that pairs two fields. To time the PARENT commit's comoments, run
      the script a second time with MDB_HIP_LIBRARY pointing at a library built from the parent: a library without the
      derived entry points measures (a) and (b) only (--label names the run in the output);
  (b) mdb_grid_batch_range_dev of x with timestamps + the values-only range grid of y: the floor of the plan a user has
      today (both fields rebuilt in HBM), before any reduction.
Batches and requests: those of scripts/profile_comoments.py (MEASUREMENTS.md section 22) - bench.py's synthetic series
(1 ms interval, chunks of 65 536 points; x relative 1 %, y another seed under relative 5 %), one group per series, and
the mixed series of tests/datagen.py lossless for both fields; about 2 000 buckets over the data (a screen), and buckets
of 7 intervals. Each figure: a warm-up call, then --samples samples, each the mean of --repeats calls between device
synchronisations; the figure is the median of the samples, given with the smallest and the largest, beside the kernels'
HIP-event times and launches of one more profiled call. Run the script more than once to see the spread between
processes. The claim to test: on "bench, screen" derived_buckets_dev is faster than (a) by more than the 7 % spread
between processes. Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_derived.py [--series N] [--points P] [--repeats R] [--samples S]"""
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

COPY_RATE_GBS = 6290.0   # the measured float4 copy rate of an MI355X (read + write bytes per second; 79 % of the 8 TB/s peak)


def measure(ctx, name, x, y, groups, n_groups, interval, repeats, has_derived):
    dev_x, dev_y = ctx.upload_segments(x), ctx.upload_segments(y)
    n_points = ctx.grid_count_range_dev(dev_x, I64_MIN, I64_MAX)
    assert n_points == ctx.grid_count_range_dev(dev_y, I64_MIN, I64_MAX)
    first, last = int(x.start_time.min()), int(x.end_time.max())
    result = {"batch": name, "segments_x": len(x), "segments_y": len(y), "points": n_points, "groups": n_groups,
              "rows_per_segment_x": round(n_points / len(x), 1), "requests": []}
    out_ts, out_val, out_y = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * (n_points + 4)), ctx.dev_alloc(4 * n_points)
    dev_groups = ctx.upload_array(groups)
    spread = lambda figure: f"{figure[0]:9.3f} ms [{figure[2][0]:.3f} .. {figure[2][1]:.3f}]"
    try:
        rebuild = timed(ctx, both(
            lambda: ctx.grid_batch_range_dev(dev_x, I64_MIN, I64_MAX, out_ts, out_val, n_points),
            lambda: ctx.grid_batch_range_dev(dev_y, I64_MIN, I64_MAX, None, out_y, n_points)), repeats)
        result.update(rebuild_both_ms=round(rebuild[0], 4), rebuild_both_range_ms=rebuild[2], rebuild_kernels=rebuild[1])
        if has_derived:
            expr = mdb.derived_expr("product")
            for label, pointer in (("aligned", out_val), ("one_float_off", out_val + 4)):
                values = timed(ctx, lambda: ctx.derived_values_dev(dev_x, dev_y, expr, I64_MIN, I64_MAX, None, pointer,
                                                                   n_points), repeats)
                kernel_ms = values[1].get("k_derived_values", [0, 0.0])[1]
                # (the elementwise kernel reads 4 + 4 B and writes 4 B per row; the two grids write 4 + 4 B before it)
                result[f"values_dev_{label}"] = {
                    "ms": round(values[0], 4), "range_ms": values[2], "kernels": values[1],
                    "k_derived_values_bytes_per_row": 12,
                    "k_derived_values_gb_per_s": round(12 * n_points / (kernel_ms * 1e-3) / 1e9, 1) if kernel_ms else None,
                    "fraction_of_copy_rate": round(12 * n_points / (kernel_ms * 1e-3) / 1e9 / COPY_RATE_GBS, 3) if kernel_ms else None}
                print(f"{name:28s} values_dev {label:14s} {spread(values)}  k_derived_values {kernel_ms:8.3f} ms "
                      f"({result[f'values_dev_{label}']['k_derived_values_gb_per_s']} GB/s)", flush=True)
        for label, width in (("screen", (last - first) // 2000 + 1), ("7_intervals", 7 * interval)):
            n_buckets = (last - first) // width + 1
            request = mdb._abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, 0)
            entry = {"request": label, "width": width, "n_buckets": n_buckets, "cells": n_groups * n_buckets}
            dev_cells = ctx.upload_array(mdb.fresh_comoments_cells((n_groups, n_buckets)))
            comoments = timed(ctx, lambda: ctx._check(ctx.lib.mdb_comoments_buckets_dev(
                ctx.handle, ctypes.byref(dev_x.seg), ctypes.byref(dev_y.seg), ctypes.c_void_p(dev_groups),
                ctypes.byref(request), ctypes.c_void_p(dev_cells))), repeats)
            ctx.dev_free(dev_cells)
            entry.update(comoments_ms=round(comoments[0], 4), comoments_range_ms=comoments[2], comoments_kernels=comoments[1],
                         comoments_over_rebuild=round(comoments[0] / rebuild[0], 3))
            line = f"(a) comoments {spread(comoments)}  (b) rebuild of both fields {spread(rebuild)}"
            if has_derived:
                expr = mdb.derived_expr("product")
                cells = ctx.upload_array(mdb.fresh_derived_cells((n_groups, n_buckets)))
                derived = timed(ctx, lambda: ctx._check(ctx.lib.mdb_derived_buckets_dev(
                    ctx.handle, ctypes.byref(dev_x.seg), ctypes.byref(dev_y.seg), ctypes.c_void_p(dev_groups),
                    ctypes.byref(request), ctypes.byref(expr), ctypes.c_void_p(cells))), repeats)
                counted = int(ctx.download_array(cells, n_groups * n_buckets, mdb.DERIVED_CELL_DTYPE)["count"].sum())
                assert counted == (profile_comoments.SAMPLES * repeats + 2) * n_points, (counted, n_points)
                ctx.dev_free(cells)
                kernel_ms = sum(ms for _, ms in derived[1].values())
                entry.update(derived_ms=round(derived[0], 4), derived_range_ms=derived[2], derived_kernels=derived[1],
                             derived_kernel_ms=round(kernel_ms, 4), derived_over_comoments=round(derived[0] / comoments[0], 3),
                             derived_over_rebuild=round(derived[0] / rebuild[0], 3),
                             derived_points_per_s=round(n_points / (derived[0] * 1e-3), 1))
                line = f"derived {spread(derived)} ({kernel_ms:.3f} ms in kernels)  " + line
            result["requests"].append(entry)
            print(f"{name:28s} {label:12s} {n_buckets:9d} buckets  {line}  {n_points} points", flush=True)
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
    parser.add_argument("--repeats", type=int, default=20)
    parser.add_argument("--samples", type=int, default=9)
    parser.add_argument("--skip-mixed", action="store_true")
    parser.add_argument("--label", default="this commit")
    a = parser.parse_args()
    profile_comoments.SAMPLES = a.samples
    ctx = mdb.Context(0)
    has_derived = hasattr(ctx.lib, "mdb_derived_buckets_dev")
    fields = []
    for seed, eb in ((SEED, mdb.error_bound("relative", 1.0)), (SEED ^ 0x5A5A5A5A, mdb.error_bound("relative", 5.0))):
        values = ctx.dev_alloc(4 * a.series * a.points)
        ctx.synth_values_dev(values, 0, a.series, a.points, seed)
        fields.append(fitted_batch(ctx, values, a.series, a.points, eb, 1000))
    results = [measure(ctx, f"bench {a.series}x{a.points}", fields[0][0], fields[1][0], fields[0][1], a.series, 1000,
                       a.repeats, has_derived)]
    if not a.skip_mixed:
        fields = []
        for base in (1000, 3000):
            host_values = np.concatenate([datagen.mixed_series(a.mixed_points, base + s, (1.0, 1.05) if s % 2 else None)[1]
                                          for s in range(a.mixed_series)])
            fields.append(fitted_batch(ctx, ctx.upload_array(host_values), a.mixed_series, a.mixed_points,
                                       mdb.error_bound("lossless"), 100))
        results.append(measure(ctx, f"mixed lossless {a.mixed_series}x{a.mixed_points}", fields[0][0], fields[1][0],
                               fields[0][1], a.mixed_series, 100, a.repeats, has_derived))
    print(json.dumps({"label": a.label, "library": mdb._abi.HIP_LIBRARY_PATH, "device": ctx.device_info()["name"],
                      "short_rows": getattr(mdb, "MDB_DERIVED_SHORT_ROWS", None),
                      "chunk_rows": getattr(mdb, "MDB_DERIVED_CHUNK_ROWS", None), "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
