#!/usr/bin/env python3
"""The value of a series at regular instants on segments (mdb_sample_at_dev, LINEAR) beside what a caller pays today
and beside its sibling, on the same resident batch, in one process: (a) mdb_grid_batch_dev - every point rebuilt, 12 B
per point, before the caller's searchsorted and lerp on the host start; (b) mdb_integral_buckets_dev with the same
request - the same pair count, (segment, bucket) for (segment, instant). Device forms only.
Batches: those of scripts/profile_integral.py - bench.py's synthetic series (1 ms interval, chunks of 65 536 points,
relative 1 %: almost all Swing on regular timestamps), one group per series; the mixed series of tests/datagen.py
(0.1 ms) lossless (MacaqueV streams among PMC-Mean and Swing); and MacaqueV alone (noise, lossless), where the walk
kernel is all there is. Three requests each: width = 1, 60 and 3 600 sampling intervals. max_gap is the sampling
interval. Each figure: a warm-up call, then the median of --samples samples, a sample the mean of --repeats calls
between device synchronisations (wall time, host side included), the three operators taking turns sample by sample,
with the smallest and the largest sample; beside the kernels' HIP-event times and launches of one more profiled call,
the bytes that would leave the device per call (16 B per instant and group; 12 B per point for the grid) and
k_sample_model_pairs' store rate (24 B per pair: the cell and the key) as a share of the HBM peak MEASUREMENTS.md
prices (8 000 GB/s). Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_sample.py [--series N] [--points P] [--repeats R] [--samples S]"""
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
HBM_PEAK_GBS = 8000.0
PAIR_BYTES = 24


def timed_in_turns(ctx, calls, repeats, samples):
    """{name: (median ms, {kernel: [launches, ms]} of one profiled call, [smallest, largest] sample)}: every call warmed
    up once, then `samples` rounds in which each call in turn runs `repeats` times between synchronisations."""
    for call in calls.values():
        call()
        ctx.sync()
    taken = {name: [] for name in calls}
    for _ in range(samples):
        for name, call in calls.items():
            started = time.perf_counter()
            for _ in range(repeats):
                call()
                ctx.sync()
            taken[name].append((time.perf_counter() - started) / repeats * 1e3)
    out = {}
    for name, call in calls.items():
        ctx.profile_enable(True)
        ctx.profile_reset()
        call()
        ctx.sync()
        kernels = {kernel: [launches, round(total_ms, 4)] for kernel, (launches, total_ms) in ctx.profile().items()}
        ctx.profile_enable(False)
        out[name] = (float(np.median(taken[name])), kernels, [round(min(taken[name]), 4), round(max(taken[name]), 4)])
    return out


def measure(ctx, name, batch, groups, n_groups, interval, repeats, samples):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    result = {"batch": name, "segments": len(batch), "points": n_points, "groups": n_groups,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist(), "requests": []}
    dev_groups = ctx.upload_array(groups)
    out_ts, out_val = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points)
    try:
        for factor in (1, 60, 3600):
            width = factor * interval
            n_instants = (last - first) // width + 1
            sample_request = ctx._sample_request(first, width, n_instants, n_groups, mdb.MDB_SAMPLE_LINEAR, interval)
            integral_request = ctx._integral_request(first, width, n_instants, n_groups, mdb.MDB_INTEGRAL_LINEAR, interval)
            dev_cells = ctx.upload_array(mdb.fresh_sample_cells((n_groups, n_instants)))
            dev_integral = ctx.upload_array(mdb.fresh_integral_cells((n_groups, n_instants)))
            calls = {
                "sample": lambda: ctx._check(ctx.lib.mdb_sample_at_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(sample_request),
                    ctypes.c_void_p(dev_cells))),
                "grid": lambda: ctx.grid_batch_dev(resident, out_ts, out_val, n_points),
                "integral": lambda: ctx._check(ctx.lib.mdb_integral_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(integral_request),
                    ctypes.c_void_p(dev_integral))),
            }
            runs = timed_in_turns(ctx, calls, repeats, samples)
            cells = ctx.download_array(dev_cells, n_groups * n_instants, mdb.SAMPLE_CELL_DTYPE)
            # (every call merged the batch once more; every series spans [first, last] without a gap, so each of its
            # instants received one contribution per call)
            n_calls = samples * repeats + 2
            assert int(cells["count"].sum()) == n_calls * n_groups * n_instants, (name, factor)
            for pointer in (dev_cells, dev_integral):
                ctx.dev_free(pointer)
            pairs = n_groups * n_instants
            model_ms = runs["sample"][1].get("k_sample_model_pairs", [0, 0.0])[1]
            entry = {"width_in_intervals": factor, "width": width, "n_instants": n_instants, "cells": pairs,
                     "sample_bytes_out": 16 * pairs, "grid_bytes_out": 12 * n_points}
            for key, run in runs.items():
                entry.update({f"{key}_ms": round(run[0], 4), f"{key}_spread": run[2], f"{key}_kernels": run[1],
                              f"{key}_kernel_ms": round(sum(ms for _, ms in run[1].values()), 4)})
            entry.update(sample_over_grid=round(runs["sample"][0] / runs["grid"][0], 3),
                         sample_over_integral=round(runs["sample"][0] / runs["integral"][0], 3),
                         model_pairs_store_gbs=round(PAIR_BYTES * pairs / (model_ms * 1e-3) / 1e9, 1) if model_ms else None,
                         model_pairs_share_of_hbm=round(PAIR_BYTES * pairs / (model_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                         if model_ms else None)
            result["requests"].append(entry)
            print(f"{name:30s} width {factor:5d} x  {n_instants:9d} instants  sample {runs['sample'][0]:8.3f} ms "
                  f"{runs['sample'][2]}  (a) grid {runs['grid'][0]:8.3f} ms {runs['grid'][2]}  (b) integral "
                  f"{runs['integral'][0]:8.3f} ms {runs['integral'][2]}  kernels: sample {entry['sample_kernel_ms']:.3f} grid "
                  f"{entry['grid_kernel_ms']:.3f} integral {entry['integral_kernel_ms']:.3f} ms  out: "
                  f"{entry['sample_bytes_out']} B against {entry['grid_bytes_out']} B  model pairs "
                  f"{entry['model_pairs_store_gbs']} GB/s", flush=True)
            print(f"{'':30s} sample kernels: {runs['sample'][1]}", flush=True)
    finally:
        for pointer in (dev_groups, out_ts, out_val):
            ctx.dev_free(pointer)
        resident.free()
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--series", type=int, default=10)
    parser.add_argument("--points", type=int, default=10_000_000)
    parser.add_argument("--mixed-series", type=int, default=16)
    parser.add_argument("--mixed-points", type=int, default=1_000_000)
    parser.add_argument("--repeats", type=int, default=10)
    parser.add_argument("--samples", type=int, default=7)
    parser.add_argument("--skip-mixed", action="store_true")
    a = parser.parse_args()
    ctx = mdb.Context(0)
    values = ctx.dev_alloc(4 * a.series * a.points)
    ctx.synth_values_dev(values, 0, a.series, a.points, SEED)
    batch, groups = fitted_batch(ctx, values, a.series, a.points, mdb.error_bound("relative", 1.0), 1000)
    results = [measure(ctx, f"bench {a.series}x{a.points}", batch, groups, a.series, 1000, a.repeats, a.samples)]
    if not a.skip_mixed:
        host_values = np.concatenate([datagen.mixed_series(a.mixed_points, 1000 + s, (1.0, 1.05) if s % 2 else None)[1]
                                      for s in range(a.mixed_series)])
        batch, groups = fitted_batch(ctx, ctx.upload_array(host_values), a.mixed_series, a.mixed_points,
                                     mdb.error_bound("lossless"), 100)
        results.append(measure(ctx, f"mixed lossless {a.mixed_series}x{a.mixed_points}", batch, groups, a.mixed_series,
                               100, a.repeats, a.samples))
        noise = np.random.default_rng(7).normal(100.0, 10.0, a.mixed_series * a.mixed_points).astype(np.float32)
        batch, groups = fitted_batch(ctx, ctx.upload_array(noise), a.mixed_series, a.mixed_points,
                                     mdb.error_bound("lossless"), 100)
        results.append(measure(ctx, f"MacaqueV noise {a.mixed_series}x{a.mixed_points}", batch, groups, a.mixed_series,
                               100, a.repeats, a.samples))
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
