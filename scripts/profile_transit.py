#!/usr/bin/env python3
"""Transitions between value cells on segments (mdb_transit_buckets_dev) beside its two neighbours on the same resident
batch, in one process and in ALTERNATING blocks: mdb_change_buckets_dev with the same request, and mdb_dwell_buckets_dev
with the same request and edges. A sample is the mean of --repeats calls of one operator between device
synchronisations, then the same of the next, --samples times over; the figure is the median sample, with the smallest
and the largest beside it. Edge lists of 1, 16 and 63 edges through the data's range, about 2 000 buckets over the data
(a screen); max_gap is the sampling interval; one group per series.
Batches: those of scripts/profile_dwell.py - bench.py's synthetic series (1 ms interval, chunks of 65 536 points,
relative 1 %: almost all Swing on regular timestamps); and the mixed series of tests/datagen.py (0.1 ms) lossless
(MacaqueV streams: one lane per stream).
Checked after every request: every call added the batch once more, so the counters of a (group, bucket) row must sum to
the change operator's accumulated `count` of that row (the same number of calls), and all of them to calls x (points -
series); one more call into fresh counters must give exactly 1 / calls of the accumulated ones.
Beside every wall time: the kernels' HIP-event times and launches of one more profiled call, and the bytes of the
counters (what leaves the device when the host wants them). Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_transit.py [--series N] [--points P] [--repeats R] [--samples S]"""
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
import profile_change  # noqa: E402
from profile_dwell import edges_between  # noqa: E402
from profile_moments import SEED, fitted_batch  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def measure(ctx, name, batch, groups, n_groups, interval, repeats):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    lo, hi = float(np.nanmin(batch.min_value)), float(np.nanmax(batch.max_value))
    result = {"batch": name, "segments": len(batch), "points": n_points, "groups": n_groups,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist(), "requests": []}
    dev_groups = ctx.upload_array(groups)
    width = (last - first) // 2000 + 1
    n_buckets = (last - first) // width + 1
    try:
        for n_edges in (1, 16, 63):
            edges = edges_between(lo, hi, n_edges)
            assert len(edges) == n_edges
            n_cells = n_edges + 1
            transit_request = ctx._transit_request(first, width, n_buckets, n_groups, interval)
            change_request = ctx._change_request(first, width, n_buckets, n_groups, interval)
            dwell_request = ctx._dwell_request(first, width, n_buckets, n_groups, interval)
            rows = n_groups * n_buckets
            dev_transit = ctx.upload_array(np.zeros(rows * n_cells * n_cells, dtype=np.uint64))
            dev_dwell = ctx.upload_array(np.zeros(rows * n_cells, dtype=np.uint64))
            dev_change = ctx.upload_array(mdb.fresh_change_cells((n_groups, n_buckets)))
            e = edges.ctypes.data_as(ctypes.c_void_p)

            def transit_call(counters=dev_transit):
                ctx._check(ctx.lib.mdb_transit_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(transit_request), e,
                    n_edges, ctypes.c_void_p(counters)))

            runs = profile_change.alternating(ctx, {
                "transit": transit_call,
                "change": lambda: ctx._check(ctx.lib.mdb_change_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(change_request),
                    ctypes.c_void_p(dev_change))),
                "dwell": lambda: ctx._check(ctx.lib.mdb_dwell_buckets_dev(
                    ctx.handle, ctypes.byref(resident.seg), ctypes.c_void_p(dev_groups), ctypes.byref(dwell_request), e,
                    n_edges, ctypes.c_void_p(dev_dwell)))}, repeats)
            calls = profile_change.SAMPLES * repeats + 2
            counts = ctx.download_array(dev_transit, rows * n_cells * n_cells, np.uint64).reshape(n_groups, n_buckets, n_cells, n_cells)
            cells = ctx.download_array(dev_change, rows, mdb.CHANGE_CELL_DTYPE).reshape(n_groups, n_buckets)
            assert int(cells["count"].sum()) == calls * (n_points - n_groups), name
            assert np.array_equal(counts.sum(axis=(2, 3), dtype=np.uint64), cells["count"]), name   # promise (a), every row
            dev_once = ctx.upload_array(np.zeros(rows * n_cells * n_cells, dtype=np.uint64))
            transit_call(dev_once)
            ctx.sync()
            once = ctx.download_array(dev_once, rows * n_cells * n_cells, np.uint64).reshape(counts.shape)
            assert np.array_equal(once * np.uint64(calls), counts), name                            # every call added the same
            off_diagonal = int(once.sum()) - int(np.trace(once, axis1=2, axis2=3).sum())
            for pointer in (dev_transit, dev_dwell, dev_change, dev_once):
                ctx.dev_free(pointer)
            entry = {"edges": n_edges, "width": width, "n_buckets": n_buckets, "counters": rows * n_cells * n_cells,
                     "bytes_leaving_the_device": 8 * rows * n_cells * n_cells, "pairs": int(once.sum()),
                     "pairs_off_the_diagonal": off_diagonal, "non_zero_counters": int((once > 0).sum())}
            for key, run in runs.items():
                entry.update({f"{key}_ms": round(run[0], 4), f"{key}_spread": run[2], f"{key}_kernels": run[1],
                              f"{key}_kernel_ms": round(sum(ms for _, ms in run[1].values()), 4)})
            result["requests"].append(entry)
            print(f"{name:30s} {n_edges:3d} edges {n_buckets:5d} buckets  transit {runs['transit'][0]:8.3f} ms {runs['transit'][2]}  "
                  f"change {runs['change'][0]:8.3f} ms {runs['change'][2]}  dwell {runs['dwell'][0]:8.3f} ms {runs['dwell'][2]}  "
                  f"kernels: transit {entry['transit_kernel_ms']:.3f} change {entry['change_kernel_ms']:.3f} dwell "
                  f"{entry['dwell_kernel_ms']:.3f} ms  {len(batch)} segments {n_points} points, {off_diagonal} of "
                  f"{int(once.sum())} pairs off the diagonal", flush=True)
            print(f"{'':30s} transit kernels {runs['transit'][1]}", flush=True)
            print(f"{'':30s} change kernels {runs['change'][1]}", flush=True)
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
    profile_change.SAMPLES = a.samples
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
