#!/usr/bin/env python3
"""Episodes on segments (mdb_episodes_dev) beside the two routes a caller had before it, with the same filter on the
same resident batch, in one process: (a) mdb_grid_batch_filter_dev - every passing point materialised (12 B each; the
islands would still have to be found on them); (b) mdb_mask_filter_dev plus the download of the mask (the runs of its
bits would still have to be found on the host, and it has no timestamps and no values).
Batches: those of scripts/profile_moments.py - bench.py's synthetic series (1 ms interval, chunks of 65 536 points,
relative 1 %: almost all Swing on regular timestamps), one group per series; and the mixed series of tests/datagen.py
(0.1 ms) lossless (its MacaqueV segments go the per-point way). Three predicates each, their thresholds
taken from the quantiles of the first series' values: almost always true (v >= the 2 % quantile), near the median
(v >= the 50 % quantile), almost never true (v >= the 98 % quantile). max_gap is the sampling interval. Each figure: a
warm-up call, then the median of --samples samples, a sample the mean of --repeats calls between device
synchronisations (wall time, host side included), with the smallest and the largest sample, beside the kernels'
HIP-event times of one more profiled call. Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_episodes.py [--series N] [--points P] [--repeats R] [--samples S]"""
import argparse
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


def measure(ctx, name, batch, groups, n_groups, interval, points_per_series, repeats):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    result = {"batch": name, "segments": len(batch), "points": n_points, "groups": n_groups,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist(), "predicates": []}
    out_ts, out_val = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points)
    words = mdb.mask_words(n_points)
    mask = ctx.dev_alloc(8 * max(words, 1))
    dev_groups = ctx.upload_array(groups)
    try:
        ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, out_ts, out_val, n_points)
        sample = ctx.download_array(out_val, min(points_per_series, n_points), np.float32)
        for label, quantile in (("almost_always", 0.02), ("median", 0.5), ("almost_never", 0.98)):
            flt = mdb.value_filter(lo=float(np.quantile(sample, quantile)))
            rule = {"max_gap": interval}
            n_episodes, n_rows, n_passing = ctx.episodes_count_dev(resident, flt, dev_groups, n_groups, **rule)
            out = ctx.dev_alloc(64 * max(n_episodes, 1))
            episodes = profile_trend.timed(ctx, lambda: ctx.episodes_into_dev(resident, flt, out, n_episodes, dev_groups,
                                                                               n_groups, **rule), repeats)
            longest = int(ctx.download_array(out, n_episodes, mdb.EPISODE_DTYPE)["count"].max()) if n_episodes else 0
            ctx.dev_free(out)
            assert ctx.grid_count_filter_dev(resident, flt) == n_passing
            points = profile_trend.timed(ctx, lambda: ctx.grid_filter_dev(resident, flt, out_ts, out_val, n_points), repeats)

            def mask_route():
                ctx.mask_filter_dev(resident, flt, mask, words)
                ctx.download_array(mask, words * 8, np.uint8)
            masks = profile_trend.timed(ctx, mask_route, repeats)
            result["predicates"].append({
                "predicate": label, "episodes": n_episodes, "rows": n_rows, "passing": n_passing, "longest_episode": longest,
                "bytes_out": {"episodes": 64 * n_episodes, "filtered_points": 12 * n_passing, "mask": 8 * words},
                "episodes_ms": round(episodes[0], 4), "episodes_spread": episodes[2], "episodes_kernels": episodes[1],
                "filter_points_ms": round(points[0], 4), "filter_points_spread": points[2], "filter_points_kernels": points[1],
                "mask_and_download_ms": round(masks[0], 4), "mask_and_download_spread": masks[2], "mask_kernels": masks[1],
                "episodes_over_filter_points": round(episodes[0] / points[0], 3),
                "episodes_over_mask_and_download": round(episodes[0] / masks[0], 3)})
            print(f"{name:28s} {label:14s} {n_episodes:9d} episodes of {n_passing:10d} passing rows (longest {longest})  "
                  f"episodes {episodes[0]:8.3f} ms {episodes[2]}  (a) filtered points {points[0]:8.3f} ms {points[2]}  "
                  f"(b) mask + download {masks[0]:8.3f} ms {masks[2]}", flush=True)
    finally:
        for pointer in (out_ts, out_val, mask, dev_groups):
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
    parser.add_argument("--samples", type=int, default=9)
    parser.add_argument("--skip-mixed", action="store_true")
    a = parser.parse_args()
    profile_trend.SAMPLES = a.samples
    ctx = mdb.Context(0)
    values = ctx.dev_alloc(4 * a.series * a.points)
    ctx.synth_values_dev(values, 0, a.series, a.points, SEED)
    batch, groups = fitted_batch(ctx, values, a.series, a.points, mdb.error_bound("relative", 1.0), 1000)
    results = [measure(ctx, f"bench {a.series}x{a.points}", batch, groups, a.series, 1000, a.points, a.repeats)]
    if not a.skip_mixed:
        host_values = np.concatenate([datagen.mixed_series(a.mixed_points, 1000 + s, (1.0, 1.05) if s % 2 else None)[1]
                                      for s in range(a.mixed_series)])
        batch, groups = fitted_batch(ctx, ctx.upload_array(host_values), a.mixed_series, a.mixed_points,
                                     mdb.error_bound("lossless"), 100)
        results.append(measure(ctx, f"mixed lossless {a.mixed_series}x{a.mixed_points}", batch, groups, a.mixed_series, 100,
                               a.mixed_points, a.repeats))
    print(json.dumps({"device": ctx.device_info()["name"], "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
