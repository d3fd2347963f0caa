#!/usr/bin/env python3
"""The time spent per value cell on segments (mdb_dwell_buckets_dev) beside its two parents on the same resident batch,
in one process and in ALTERNATING blocks: mdb_hist_buckets_dev with the same edges and buckets, and
mdb_integral_buckets_dev under STEP with the same request. A sample is the mean of --repeats calls of one operator
between device synchronisations, then the same of the next, --samples times over; the figure is the median sample, with
the smallest and the largest beside it. Edge lists of 1, 16 and 4 095 edges through the data's range.
Batches and bucket widths: those of scripts/profile_change.py and scripts/profile_integral.py - bench.py's synthetic
series (1 ms interval, chunks of 65 536 points, relative 1 %: almost all Swing on regular timestamps), one group per
series; and the mixed series of tests/datagen.py (0.1 ms) lossless (MacaqueV streams: one lane per stream). One request
each: about 2 000 buckets over the data (a screen) - with 4 095 edges about 250, so that the counters stay within
100 MB. max_gap is the sampling interval.
Today's alternative is timed once beside them: grid() of the resident batch to the host (12 bytes a point over PCIe),
then a numpy pass - the cell of every row's value, the bucket of every row and its successor, np.bincount for the
intervals that stay inside one bucket and a Python loop over those that cross an edge.
Beside every wall time: the kernels' HIP-event times and launches of one more profiled call, and the bytes that leave
the device. Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_dwell.py [--series N] [--points P] [--repeats R] [--samples S]"""
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
import profile_change  # noqa: E402
from profile_moments import SEED, fitted_batch  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def keys_of(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def edges_between(lo, hi, n_edges):
    keys = np.unique(np.linspace(int(keys_of(np.float32(lo))), int(keys_of(np.float32(hi))), n_edges + 2)[1:-1].astype(np.int64))
    return (keys ^ ((keys >> 31) & 0x7FFFFFFF)).astype(np.int32).view(np.float32)


def numpy_alternative(ctx, resident, series_points, edges, origin, width, n_buckets, interval):
    """grid() to the host, then the numpy pass of one group per series; returns (seconds of grid, seconds of numpy,
    dwell)."""
    started = time.perf_counter()
    timestamps, values = ctx.grid_resident(resident)
    grid_s = time.perf_counter() - started
    started = time.perf_counter()
    n_cells = len(edges) + 1
    n_groups = len(timestamps) // series_points
    cell = np.searchsorted(keys_of(edges), keys_of(values), side="right")
    group = np.arange(len(timestamps)) // series_points
    step = np.diff(timestamps)
    linked = np.flatnonzero((group[1:] == group[:-1]) & (step > 0) & (step <= interval))
    t0, t1 = timestamps[linked], timestamps[linked + 1]
    b0, b1 = (t0 - origin) // width, (t1 - 1 - origin) // width
    inside = (b0 == b1) & (b0 >= 0) & (b0 < n_buckets)
    # (np.bincount sums its weights in f64: exact here, a batch's linked time being far below 2^53 microseconds)
    dwell = np.bincount((group[linked][inside] * n_buckets + b0[inside]) * n_cells + cell[linked][inside],
                        weights=(t1 - t0)[inside], minlength=n_groups * n_buckets * n_cells).astype(np.uint64)
    for k in np.flatnonzero(b0 != b1):   # the intervals a bucket edge cuts
        for b in range(max(int(b0[k]), 0), min(int(b1[k]), n_buckets - 1) + 1):
            a, e = max(int(t0[k]), origin + b * width), min(int(t1[k]), origin + (b + 1) * width)
            dwell[(int(group[linked[k]]) * n_buckets + b) * n_cells + int(cell[linked[k]])] += e - a
    return grid_s, time.perf_counter() - started, dwell.reshape(n_groups, n_buckets, n_cells), 12 * len(timestamps)


def measure(ctx, name, batch, groups, n_groups, series_points, interval, repeats, alternative):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    lo, hi = float(np.nanmin(batch.min_value)), float(np.nanmax(batch.max_value))
    result = {"batch": name, "segments": len(batch), "points": n_points, "groups": n_groups,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist(), "requests": []}
    dev_groups = ctx.upload_array(groups)
    try:
        for n_edges in (1, 16, mdb.MDB_HIST_MAX_EDGES):
            edges = edges_between(lo, hi, n_edges)
            assert len(edges) == n_edges
            width = (last - first) // (2000 if n_edges <= 16 else 250) + 1
            n_buckets = (last - first) // width + 1
            n_cells = n_edges + 1
            dwell_request = ctx._dwell_request(first, width, n_buckets, n_groups, interval)
            integral_request = ctx._integral_request(first, width, n_buckets, n_groups, mdb.MDB_INTEGRAL_STEP, interval)
            bucket_request = ctx._bucket_request(first, width, n_buckets, n_groups, None, None, 0)
            counters = n_groups * n_buckets * n_cells
            dev_dwell = ctx.upload_array(np.zeros(counters, dtype=np.uint64))
            dev_hist = ctx.upload_array(np.zeros(counters, dtype=np.uint64))
            dev_integral = ctx.upload_array(mdb.fresh_integral_cells((n_groups, n_buckets)))
            e = edges.ctypes.data_as(ctypes.c_void_p)
            runs = profile_change.alternating(ctx, {
                "dwell": lambda: ctx._check(ctx.lib.mdb_dwell_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(dwell_request), e,
                    n_edges, ctypes.c_void_p(dev_dwell))),
                "hist": lambda: ctx._check(ctx.lib.mdb_hist_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(bucket_request), e,
                    n_edges, ctypes.c_void_p(dev_hist))),
                "integral": lambda: ctx._check(ctx.lib.mdb_integral_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(integral_request),
                    ctypes.c_void_p(dev_integral)))}, repeats)
            # (every call added the batch once more: each series' linked time is its points less one, an interval each)
            calls = profile_change.SAMPLES * repeats + 2
            dwell = ctx.download_array(dev_dwell, counters, np.uint64).reshape(n_groups, n_buckets, n_cells)
            cells = ctx.download_array(dev_integral, n_groups * n_buckets, mdb.INTEGRAL_CELL_DTYPE).reshape(n_groups, n_buckets)
            assert int(dwell.sum()) == calls * (n_points - n_groups) * interval, name
            assert np.array_equal(dwell.sum(axis=2, dtype=np.uint64), cells["duration"]), name
            hist = ctx.download_array(dev_hist, counters, np.uint64)
            assert int(hist.sum()) == calls * n_points, name
            for pointer in (dev_dwell, dev_hist, dev_integral):
                ctx.dev_free(pointer)
            entry = {"edges": n_edges, "width": width, "n_buckets": n_buckets, "counters": counters,
                     "bytes_leaving_the_device": 8 * counters}
            for key, run in runs.items():
                entry.update({f"{key}_ms": round(run[0], 4), f"{key}_spread": run[2], f"{key}_kernels": run[1],
                              f"{key}_kernel_ms": round(sum(ms for _, ms in run[1].values()), 4)})
            entry.update(dwell_over_parents=round(runs["dwell"][0] / (runs["hist"][0] + runs["integral"][0]), 3),
                         dwell_points_per_s=round(n_points / (runs["dwell"][0] * 1e-3), 1))
            if alternative and n_edges == 16:
                grid_s, numpy_s, expected, grid_bytes = numpy_alternative(ctx, resident, series_points, edges, first, width,
                                                                          n_buckets, interval)
                assert np.array_equal(expected * np.uint64(calls), dwell), name
                entry.update(alternative_grid_ms=round(grid_s * 1e3, 2), alternative_numpy_ms=round(numpy_s * 1e3, 2),
                             alternative_bytes_leaving_the_device=grid_bytes)
            result["requests"].append(entry)
            print(f"{name:30s} {n_edges:5d} edges {n_buckets:6d} buckets  dwell {runs['dwell'][0]:8.3f} ms {runs['dwell'][2]}  "
                  f"hist {runs['hist'][0]:8.3f} ms {runs['hist'][2]}  integral step {runs['integral'][0]:8.3f} ms "
                  f"{runs['integral'][2]}  kernels: dwell {entry['dwell_kernel_ms']:.3f} hist {entry['hist_kernel_ms']:.3f} "
                  f"integral {entry['integral_kernel_ms']:.3f} ms  {len(batch)} segments {n_points} points", flush=True)
            print(f"{'':30s} dwell kernels {runs['dwell'][1]}  alternative: "
                  f"{ {k: v for k, v in entry.items() if k.startswith('alternative')} }", flush=True)
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
    parser.add_argument("--skip-alternative", action="store_true")
    a = parser.parse_args()
    profile_change.SAMPLES = a.samples
    ctx = mdb.Context(0)
    values = ctx.dev_alloc(4 * a.series * a.points)
    ctx.synth_values_dev(values, 0, a.series, a.points, SEED)
    batch, groups = fitted_batch(ctx, values, a.series, a.points, mdb.error_bound("relative", 1.0), 1000)
    results = [measure(ctx, f"bench {a.series}x{a.points}", batch, groups, a.series, a.points, 1000, a.repeats,
                       not a.skip_alternative)]
    if not a.skip_mixed:
        host_values = np.concatenate([datagen.mixed_series(a.mixed_points, 1000 + s, (1.0, 1.05) if s % 2 else None)[1]
                                      for s in range(a.mixed_series)])
        batch, groups = fitted_batch(ctx, ctx.upload_array(host_values), a.mixed_series, a.mixed_points,
                                     mdb.error_bound("lossless"), 100)
        results.append(measure(ctx, f"mixed lossless {a.mixed_series}x{a.mixed_points}", batch, groups, a.mixed_series,
                               a.mixed_points, 100, a.repeats, not a.skip_alternative))
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
