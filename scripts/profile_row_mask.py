#!/usr/bin/env python3
"""Row masks (mdb_mask_filter_dev, mdb_agg_batch_mask_dev, mdb_grid_batch_mask_dev, mdb_*_where*) against what the
library offered before them for `SELECT agg(b) FROM t WHERE a >= q`, on two field columns of the same series:
  * mask_filter_dev(a) + agg_batch_mask_dev(b) against mdb_grid_batch_range_dev of both fields into HBM (timestamps and
    values of a, values only of b) - a LOWER bound of the old cost: the filtering and folding are still to be done;
  * agg_batch_mask_dev with a full mask against mdb_agg_batch_range_dev, and mask_filter_dev against
    mdb_grid_count_filter_dev: what going through a bitmap costs;
  * mask_filter_dev(a) + grid_batch_mask_dev(b) (the selected rows of b into HBM);
  * agg_where / grid_where from host batches, with the bytes copied down per selected row.
Batches: bench.py's synthetic series (1 ms interval, chunks of 65 536 points, relative 1 %: about 99.6 % Swing on
regular timestamps), two fields from two seeds, fitted by compress_chunks_dev; and the mixed series of tests/datagen.py
(0.1 ms, relative 1 %), two fields from two seeds. Selectivities 1, 50 and 100 %: `a >= q` with q the (1 - s) quantile
of a sample of a's rebuilt points. Each figure: a warm-up call, then the MEDIAN of --repeats calls between device
synchronisations, with the kernels' HIP-event times (mdb_profile_*) of one more profiled call. Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_row_mask.py [--series N] [--points P] [--repeats R]"""
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
SELECTIVITIES = (0.01, 0.50, 1.0)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def timed(ctx, call, repeats):
    """(median ms over `repeats` synchronised calls, {kernel: ms} of one profiled call)."""
    call()
    ctx.sync()
    times = []
    for _ in range(repeats):
        started = time.perf_counter()
        call()
        ctx.sync()
        times.append((time.perf_counter() - started) * 1e3)
    ctx.profile_enable(True)
    ctx.profile_reset()
    call()
    ctx.sync()
    kernels = {name: round(total_ms, 4) for name, (_, total_ms) in ctx.profile().items()}
    ctx.profile_enable(False)
    return float(np.median(times)), kernels


def thresholds(ctx, resident, n_points, out_ts, out_val):
    ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, out_ts, out_val, n_points)
    step = max(n_points // (1 << 20), 1)
    sample = np.concatenate([ctx.download_array(out_val, min(4096, n_points - k), np.float32, k)
                             for k in range(0, n_points, step * 4096)])
    sample = np.sort(sample[np.isfinite(sample)])
    return [(s, mdb.value_filter(lo=-np.inf) if s == 1.0 else
             mdb.value_filter(lo=float(sample[int((1.0 - s) * (len(sample) - 1))]))) for s in SELECTIVITIES]


def measure(ctx, name, field_a, field_b, repeats, host_forms):
    dev_a, dev_b = ctx.upload_segments(field_a), ctx.upload_segments(field_b)
    n_points = ctx.grid_count_range_dev(dev_a, I64_MIN, I64_MAX)
    assert n_points == ctx.grid_count_range_dev(dev_b, I64_MIN, I64_MAX), "the fields do not line up"
    out_ts, out_val, out_val_b = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points), ctx.dev_alloc(4 * n_points)
    words = mdb.mask_words(n_points)
    mask = ctx.dev_alloc(8 * max(words, 1))
    result = {"batch": name, "points": n_points, "segments": [len(field_a), len(field_b)],
              "model_types": [np.bincount(f.model_type_id.astype(np.int64), minlength=3).tolist() for f in (field_a, field_b)]}
    try:
        def both_grids():
            ctx.grid_batch_range_dev(dev_a, I64_MIN, I64_MAX, out_ts, out_val, n_points)
            ctx.grid_batch_range_dev(dev_b, I64_MIN, I64_MAX, None, out_val_b, n_points)
        grids = timed(ctx, both_grids, repeats)
        range_agg = timed(ctx, lambda: ctx.agg_batch_range_dev(dev_b, I64_MIN, I64_MAX, MASK), repeats)
        result.update(range_grid_both_fields_ms=round(grids[0], 4), range_grid_kernels_ms=grids[1],
                      range_agg_ms=round(range_agg[0], 4), range_agg_kernels_ms=range_agg[1])
        runs = []
        for selectivity, flt in thresholds(ctx, dev_a, n_points, out_ts, out_val):
            _, n_set = ctx.mask_filter_dev(dev_a, flt, mask, words)
            produce = timed(ctx, lambda: ctx.mask_filter_dev(dev_a, flt, mask, words), repeats)
            count_filter = timed(ctx, lambda: ctx.grid_count_filter_dev(dev_a, flt), repeats)
            agg = timed(ctx, lambda: ctx.agg_mask_dev(dev_b, I64_MIN, I64_MAX, mask, n_points, MASK), repeats)
            grid = timed(ctx, lambda: ctx.grid_mask_dev(dev_b, I64_MIN, I64_MAX, mask, n_points, out_ts, out_val, n_points),
                         repeats)
            run = {"selectivity": selectivity, "selected": n_set,
                   "mask_filter_ms": round(produce[0], 4), "mask_filter_kernels_ms": produce[1],
                   "grid_count_filter_ms": round(count_filter[0], 4),
                   "mask_filter_x_grid_count_filter": round(produce[0] / count_filter[0], 3),
                   "agg_mask_ms": round(agg[0], 4), "agg_mask_kernels_ms": agg[1],
                   "agg_mask_x_range_agg": round(agg[0] / range_agg[0], 3),
                   "mask_filter_plus_agg_mask_ms": round(produce[0] + agg[0], 4),
                   "mask_filter_plus_agg_mask_x_both_grids": round((produce[0] + agg[0]) / grids[0], 4),
                   "grid_mask_ms": round(grid[0], 4), "grid_mask_kernels_ms": grid[1],
                   "mask_filter_plus_grid_mask_x_both_grids": round((produce[0] + grid[0]) / grids[0], 4)}
            if host_forms:
                agg_where = timed(ctx, lambda: ctx.agg_where([field_a], [flt], field_b, MASK), repeats)
                grid_where = timed(ctx, lambda: ctx.grid_where([field_a], [flt], field_b), repeats)
                run.update(agg_where_ms=round(agg_where[0], 4), agg_where_kernels_ms=agg_where[1],
                           grid_where_ms=round(grid_where[0], 4),
                           agg_where_bytes_down_per_selected_row=round(24 / max(n_set, 1), 6),
                           grid_where_bytes_down_per_selected_row=round((12 * n_set + 4 * len(field_b)) / max(n_set, 1), 4))
            print(f"{name:26s} sel {selectivity:4.2f}  mask {produce[0]:8.3f} ms (count_filter {count_filter[0]:7.3f})  agg_mask "
                  f"{agg[0]:8.3f} ms (range agg {range_agg[0]:7.3f})  mask+agg {produce[0] + agg[0]:8.3f} ms against both grids "
                  f"{grids[0]:8.3f} ms  grid_mask {grid[0]:8.3f} ms" +
                  (f"  agg_where {run['agg_where_ms']:8.3f} ms grid_where {run['grid_where_ms']:8.3f} ms" if host_forms else ""),
                  flush=True)
            runs.append(run)
        result["runs"] = runs
    finally:
        for pointer in (out_ts, out_val, out_val_b, mask):
            ctx.dev_free(pointer)
        dev_a.free()
        dev_b.free()
    return result


def fit(ctx, values, n_series, points, interval):
    starts = np.arange(0, points, CHUNK_POINTS, dtype=np.uint64)
    offsets = (np.arange(n_series, dtype=np.uint64)[:, None] * np.uint64(points) + starts[None, :]).reshape(-1)
    offsets = np.concatenate([offsets, np.array([n_series * points], dtype=np.uint64)])
    offsets_dev, first_index_dev = ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, n_series))
    fitted = ctx.compress_chunks_dev(0, values, offsets_dev, len(offsets) - 1, mdb.error_bound("relative", 1.0), 0, interval,
                                     first_index_dev)
    ctx.sync()
    for pointer in (values, offsets_dev, first_index_dev):
        ctx.dev_free(pointer)
    batch = fitted.download()
    fitted.free()
    return batch


def bench_shaped(ctx, a):
    fields = []
    for seed in (SEED, SEED + 1):
        values = ctx.dev_alloc(4 * a.series * a.points)
        ctx.synth_values_dev(values, 0, a.series, a.points, seed)
        fields.append(fit(ctx, values, a.series, a.points, 1000))
    return measure(ctx, f"bench {a.series}x{a.points}", fields[0], fields[1], a.repeats, True)


def mixed(ctx, a):
    fields = []
    for base in (1000, 5000):
        host_values = np.concatenate([datagen.mixed_series(a.mixed_points, base + s, (1.0, 1.05) if s % 2 else None)[1]
                                      for s in range(a.mixed_series)])
        fields.append(fit(ctx, ctx.upload_array(host_values), a.mixed_series, a.mixed_points, 100))
    return measure(ctx, f"mixed 1% {a.mixed_series}x{a.mixed_points}", fields[0], fields[1], a.repeats, False)


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
        results.append(mixed(ctx, a))
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
