#!/usr/bin/env python3
"""Value predicates pushed down to the segments (mdb_grid_*_filter*, mdb_agg_batch_filter*) against what they replace,
on the same batch:
  * filtered grid (mdb_grid_batch_filter_dev) against the range grid (mdb_grid_batch_range_dev) of a resident batch;
  * the owned filtered grid (mdb_grid_batch_filter_owned, host batch in, passing rows out) against
    mdb_grid_batch_owned plus a numpy filter, with the bytes copied back per point of the batch;
  * filtered aggregates (mdb_agg_batch_filter_dev) against the range aggregates (mdb_agg_batch_range_dev).
Batches: bench.py's synthetic series (1 ms interval, chunks of 65 536 points, relative 1 %: about 99.6 % Swing on
regular timestamps), fitted by compress_chunks_dev, and the mixed series of tests/datagen.py (0.1 ms), lossless and
relative 1 %. Selectivities 0, 1, 10, 50 and 100 %: `value >= q` with q the (1 - s) quantile of a sample of the
rebuilt points (0 %: above every value; 100 %: -inf). Each figure: a warm-up call, then the mean of --repeats calls
between device synchronisations, with the kernels' HIP-event times of one more profiled call. Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_value_filter.py [--series N] [--points P] [--repeats R]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import modelardb_rs_amd as mdb  # noqa: E402
import datagen  # noqa: E402

CHUNK_POINTS = 65536
SEED = 0x4D44425F52454631  # bench.py's
MASK = mdb.MDB_AGG_COUNT | mdb.MDB_AGG_MIN | mdb.MDB_AGG_MAX | mdb.MDB_AGG_SUM
SELECTIVITIES = (0.0, 0.01, 0.10, 0.50, 1.0)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def timed(ctx, call, repeats):
    """(mean ms over `repeats` synchronised calls, {kernel: ms} of one profiled call)."""
    call()
    ctx.sync()
    started = time.perf_counter()
    for _ in range(repeats):
        call()
        ctx.sync()
    ms = (time.perf_counter() - started) / repeats * 1e3
    ctx.profile_enable(True)
    ctx.profile_reset()
    call()
    ctx.sync()
    kernels = {name: round(total_ms, 4) for name, (_, total_ms) in ctx.profile().items()}
    ctx.profile_enable(False)
    return ms, kernels


def thresholds(ctx, resident, n_points):
    """Filters of the five selectivities from a sample of the rebuilt points."""
    out_ts, out_val = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points)
    try:
        ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, out_ts, out_val, n_points)
        step = max(n_points // (1 << 20), 1)
        sample = np.concatenate([ctx.download_array(out_val, min(4096, n_points - k), np.float32, k)
                                 for k in range(0, n_points, step * 4096)])
    finally:
        ctx.dev_free(out_ts)
        ctx.dev_free(out_val)
    sample = np.sort(sample[np.isfinite(sample)])
    out = []
    for s in SELECTIVITIES:
        if s == 0.0:
            out.append((s, mdb.value_filter(lo=float(sample[-1]) * 2.0 + 1e30)))
        elif s == 1.0:
            out.append((s, mdb.value_filter(lo=-np.inf)))
        else:
            out.append((s, mdb.value_filter(lo=float(sample[int((1.0 - s) * (len(sample) - 1))]))))
    return out


def measure(ctx, name, batch, repeats, owned):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    out_ts, out_val = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points)
    result = {"batch": name, "segments": len(batch), "points": n_points,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist()}
    try:
        grid = timed(ctx, lambda: ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, out_ts, out_val, n_points), repeats)
        agg = timed(ctx, lambda: ctx.agg_batch_range_dev(resident, I64_MIN, I64_MAX, MASK), repeats)
        result.update(range_grid_ms=round(grid[0], 4), range_grid_kernels_ms=grid[1], range_agg_ms=round(agg[0], 4),
                      range_agg_kernels_ms=agg[1])
        if owned:
            def owned_baseline():
                ts, values, _, _ = ctx.grid_batch_owned(batch)
                keep = values >= np.float32(0.0)
                return ts[keep], values[keep]
            base = timed(ctx, owned_baseline, repeats)
            result.update(owned_grid_plus_numpy_ms=round(base[0], 4),
                          owned_grid_bytes_per_point=round((12 * n_points + 4 * len(batch)) / n_points, 4))
        runs = []
        for selectivity, flt in thresholds(ctx, resident, n_points):
            n_pass = ctx.grid_count_filter_dev(resident, flt)
            fgrid = timed(ctx, lambda: ctx.grid_filter_dev(resident, flt, out_ts, out_val, n_points), repeats)
            fagg = timed(ctx, lambda: ctx.agg_filter_dev(resident, flt, MASK), repeats)
            run = {"selectivity": selectivity, "passing": n_pass, "filter_grid_ms": round(fgrid[0], 4),
                   "filter_grid_x_range_grid": round(fgrid[0] / grid[0], 3), "filter_grid_kernels_ms": fgrid[1],
                   "filter_agg_ms": round(fagg[0], 4), "filter_agg_x_range_agg": round(fagg[0] / agg[0], 3),
                   "filter_agg_kernels_ms": fagg[1]}
            if owned:
                fowned = timed(ctx, lambda: ctx.grid_filter(batch, flt), repeats)
                run.update(owned_filter_ms=round(fowned[0], 4),
                           owned_filter_bytes_per_point=round((12 * n_pass + 4 * len(batch)) / n_points, 4))
            print(f"{name:28s} sel {selectivity:5.2f}  grid {fgrid[0]:9.3f} ms (range {grid[0]:8.3f})  agg "
                  f"{fagg[0]:8.3f} ms (range {agg[0]:7.3f})" +
                  (f"  owned {run['owned_filter_ms']:9.3f} ms (grid+numpy {base[0]:9.3f})" if owned else ""), flush=True)
            runs.append(run)
        result["runs"] = runs
    finally:
        ctx.dev_free(out_ts)
        ctx.dev_free(out_val)
        resident.free()
    return result


def bench_shaped(ctx, a):
    eb = mdb.error_bound("relative", 1.0)
    total = a.series * a.points
    values = ctx.dev_alloc(4 * total)
    ctx.synth_values_dev(values, 0, a.series, a.points, SEED)
    starts = np.arange(0, a.points, CHUNK_POINTS, dtype=np.uint64)
    offsets = (np.arange(a.series, dtype=np.uint64)[:, None] * np.uint64(a.points) + starts[None, :]).reshape(-1)
    offsets = np.concatenate([offsets, np.array([total], dtype=np.uint64)])
    offsets_dev, first_index_dev = ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, a.series))
    fitted = ctx.compress_chunks_dev(0, values, offsets_dev, len(offsets) - 1, eb, 0, 1000, first_index_dev)
    ctx.sync()
    for pointer in (values, offsets_dev, first_index_dev):
        ctx.dev_free(pointer)
    batch = fitted.download()
    fitted.free()
    return measure(ctx, f"bench {a.series}x{a.points}", batch, a.repeats, True)


def mixed(ctx, a, bound):
    eb = mdb.error_bound("lossless") if bound == "lossless" else mdb.error_bound("relative", 1.0)
    points = a.mixed_points
    host_values = np.concatenate([datagen.mixed_series(points, 1000 + s, (1.0, 1.05) if s % 2 else None)[1]
                                  for s in range(a.mixed_series)])
    values = ctx.upload_array(host_values)
    starts = np.arange(0, points, CHUNK_POINTS, dtype=np.uint64)
    offsets = np.concatenate([s * points + starts for s in range(a.mixed_series)] +
                             [np.array([a.mixed_series * points], dtype=np.uint64)]).astype(np.uint64)
    offsets_dev, first_index_dev = ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, a.mixed_series))
    fitted = ctx.compress_chunks_dev(0, values, offsets_dev, len(offsets) - 1, eb, 0, 100, first_index_dev)
    ctx.sync()
    for pointer in (values, offsets_dev, first_index_dev):
        ctx.dev_free(pointer)
    batch = fitted.download()
    fitted.free()
    return measure(ctx, f"mixed {bound} {a.mixed_series}x{points}", batch, a.repeats, False)


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
    results = [bench_shaped(ctx, a)]
    if not a.skip_mixed:
        results += [mixed(ctx, a, "lossless"), mixed(ctx, a, "1%")]
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
