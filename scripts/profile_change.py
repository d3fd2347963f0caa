#!/usr/bin/env python3
"""Changes between consecutive points on segments (mdb_change_buckets_dev) beside the time-weighted operator
(mdb_integral_buckets_dev, LINEAR) with the same bucket request on the same resident batch, in one process and in
ALTERNATING blocks: a sample is the mean of --repeats calls of one operator between device synchronisations, then the
same of the other, --samples times over; the figure is the median sample, with the smallest and the largest beside it.
The two share the span, the heads and the walk over (segment, bucket) pairs; the change operator's arithmetic is
simpler and its cell is 64 bytes instead of 16.
Batches and bucket widths: those of scripts/profile_integral.py - bench.py's synthetic series (1 ms interval, chunks of
65 536 points, relative 1 %: almost all Swing on regular timestamps), one group per series; and the mixed series of
tests/datagen.py (0.1 ms) lossless (MacaqueV streams: one lane per stream). Two requests each: about 2 000 buckets over
the data (a screen), and buckets of 7 intervals (many pairs). max_gap is the sampling interval.
Then a PMC-Mean-only batch at two segment lengths with the number of segments held equal (--pmc-segments segments of
64 and of 6 400 rows, one series, a screen of about 2 000 buckets): if the operator follows the segments and not the
points, the two take the same time.
Beside every wall time: the kernels' HIP-event times and launches of one more profiled call. Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_change.py [--series N] [--points P] [--repeats R] [--samples S]"""
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
import scale_cases  # noqa: E402
from profile_moments import SEED, fitted_batch  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SAMPLES = 9


def alternating(ctx, calls, repeats):
    """{name: (median ms, {kernel: [launches, ms]}, [smallest, largest] sample)} of the calls, timed in alternating
    blocks of `repeats` synchronised calls."""
    for call in calls.values():   # warm-up: code objects, scratch
        call()
        ctx.sync()
    samples = {name: [] for name in calls}
    for _ in range(SAMPLES):
        for name, call in calls.items():
            started = time.perf_counter()
            for _ in range(repeats):
                call()
                ctx.sync()
            samples[name].append((time.perf_counter() - started) / repeats * 1e3)
    out = {}
    for name, call in calls.items():
        ctx.profile_enable(True)
        ctx.profile_reset()
        call()
        ctx.sync()
        kernels = {kernel: [launches, round(total_ms, 4)] for kernel, (launches, total_ms) in ctx.profile().items()}
        ctx.profile_enable(False)
        out[name] = (float(np.median(samples[name])), kernels, [round(min(samples[name]), 4), round(max(samples[name]), 4)])
    return out


def measure(ctx, name, batch, groups, n_groups, interval, repeats, requests=("screen", "7_intervals")):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    result = {"batch": name, "segments": len(batch), "points": n_points, "groups": n_groups,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist(), "requests": []}
    dev_groups = ctx.upload_array(groups)
    try:
        for label, width in (("screen", (last - first) // 2000 + 1), ("7_intervals", 7 * interval)):
            if label not in requests:
                continue
            n_buckets = (last - first) // width + 1
            change_request = ctx._change_request(first, width, n_buckets, n_groups, interval)
            integral_request = ctx._integral_request(first, width, n_buckets, n_groups, mdb.MDB_INTEGRAL_LINEAR, interval)
            dev_change = ctx.upload_array(mdb.fresh_change_cells((n_groups, n_buckets)))
            dev_integral = ctx.upload_array(mdb.fresh_integral_cells((n_groups, n_buckets)))
            runs = alternating(ctx, {
                "change": lambda: ctx._check(ctx.lib.mdb_change_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(change_request),
                    ctypes.c_void_p(dev_change))),
                "integral": lambda: ctx._check(ctx.lib.mdb_integral_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(integral_request),
                    ctypes.c_void_p(dev_integral)))}, repeats)
            # (every call merged the batch once more: each series' pairs are its points less one, an interval each)
            calls = SAMPLES * repeats + 2
            cells = ctx.download_array(dev_change, n_groups * n_buckets, mdb.CHANGE_CELL_DTYPE)
            assert int(cells["count"].sum()) == calls * (n_points - n_groups), name
            assert int(cells["duration"].sum()) == calls * (n_points - n_groups) * interval, name
            cells = ctx.download_array(dev_integral, n_groups * n_buckets, mdb.INTEGRAL_CELL_DTYPE)
            assert int(cells["duration"].sum()) == calls * (n_points - n_groups) * interval, name
            ctx.dev_free(dev_change)
            ctx.dev_free(dev_integral)
            entry = {"request": label, "width": width, "n_buckets": n_buckets, "cells": n_groups * n_buckets}
            for key, run in runs.items():
                entry.update({f"{key}_ms": round(run[0], 4), f"{key}_spread": run[2], f"{key}_kernels": run[1],
                              f"{key}_kernel_ms": round(sum(ms for _, ms in run[1].values()), 4)})
            entry.update(change_over_integral=round(runs["change"][0] / runs["integral"][0], 3),
                         change_points_per_s=round(n_points / (runs["change"][0] * 1e-3), 1))
            result["requests"].append(entry)
            print(f"{name:34s} {label:12s} {n_buckets:9d} buckets  change {runs['change'][0]:8.3f} ms {runs['change'][2]}  "
                  f"integral linear {runs['integral'][0]:8.3f} ms {runs['integral'][2]}  kernels: change "
                  f"{entry['change_kernel_ms']:.3f} integral {entry['integral_kernel_ms']:.3f} ms  {len(batch)} segments "
                  f"{n_points} points", flush=True)
            print(f"{'':34s} change kernels {runs['change'][1]}", flush=True)
    finally:
        ctx.dev_free(dev_groups)
        resident.free()
    return result


def pmc_batch(n_segments, length, interval, seed):
    """One series of PMC-Mean segments of `length` rows each on regular timestamps, every level another."""
    rng = np.random.default_rng(seed)
    levels = rng.normal(50.0, 20.0, n_segments).astype(np.float32)
    starts = np.arange(n_segments, dtype=np.int64) * (length * interval)
    return scale_cases.simple_batch(np.full(n_segments, scale_cases.PMC), starts, np.full(n_segments, length),
                                    np.full(n_segments, interval), levels, levels, np.zeros(n_segments, dtype=bool))


def main():
    global SAMPLES
    parser = argparse.ArgumentParser()
    parser.add_argument("--series", type=int, default=10)
    parser.add_argument("--points", type=int, default=10_000_000)
    parser.add_argument("--mixed-series", type=int, default=16)
    parser.add_argument("--mixed-points", type=int, default=1_000_000)
    parser.add_argument("--pmc-segments", type=int, default=200_000)
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
    for length in (64, 6_400):
        batch = pmc_batch(a.pmc_segments, length, 1000, 29)
        results.append(measure(ctx, f"PMC-Mean {a.pmc_segments} segments x {length} rows", batch,
                               np.zeros(len(batch), dtype=np.uint32), 1, 1000, a.repeats, requests=("screen",)))
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
