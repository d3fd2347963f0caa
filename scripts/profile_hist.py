#!/usr/bin/env python3
"""Value histograms and exact quantiles on segments (mdb_hist_batch_dev, mdb_quantile_batch_dev) against the only route
to the same answer without them: mdb_grid_batch_range_dev with values only into HBM (which still leaves the binning or
the sorting undone), on the same resident batch.
Batches: bench.py's synthetic series (1 ms interval, chunks of 65 536 points, relative 1 %: about 99.6 % Swing on
regular timestamps), fitted by compress_chunks_dev, and the mixed series of tests/datagen.py (0.1 ms), lossless and
relative 1 %. Histograms of 64 and of 4 095 edges, even in value between the 0.1 % and 99.9 % quantiles of a sample of
the rebuilt points, one group; the median. Each figure: a warm-up call, then the mean of --repeats calls between device
synchronisations, with the kernels' HIP-event times and launches of one more profiled call (the launches of k_hist of a
quantile call are its passes). Prints one JSON line.
Usage (on the GPU box): python3 scripts/profile_hist.py [--series N] [--points P] [--repeats R]"""
import argparse
import ctypes
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
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def timed(ctx, call, repeats):
    """(mean ms over `repeats` synchronised calls, {kernel: [launches, ms]} of one profiled call)."""
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
    kernels = {name: [launches, round(total_ms, 4)] for name, (launches, total_ms) in ctx.profile().items()}
    ctx.profile_enable(False)
    return ms, kernels


def measure(ctx, name, batch, repeats):
    resident = ctx.upload_segments(batch)
    n_points = ctx.grid_count_range_dev(resident, I64_MIN, I64_MAX)
    out_val = ctx.dev_alloc(4 * n_points)
    result = {"batch": name, "segments": len(batch), "points": n_points,
              "model_types": np.bincount(batch.model_type_id.astype(np.int64), minlength=3).tolist()}
    try:
        rebuild = timed(ctx, lambda: ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, None, out_val, n_points), repeats)
        step = max(n_points // (1 << 20), 1)
        sample = np.concatenate([ctx.download_array(out_val, min(4096, n_points - k), np.float32, k)
                                 for k in range(0, n_points, step * 4096)])
        sample = np.sort(sample[np.isfinite(sample)])
        low, high = float(sample[len(sample) // 1000]), float(sample[-1 - len(sample) // 1000])
        result.update(rebuild_values_ms=round(rebuild[0], 4), rebuild_kernels=rebuild[1])
        for n_edges in (64, 4095):
            edges = np.unique(np.linspace(low, high, n_edges).astype(np.float32))
            counts = np.zeros((1, len(edges) + 1), dtype=np.uint64)
            dev_counts = ctx.upload_array(counts)
            request = mdb._abi.HistRequestC(I64_MIN, I64_MAX, len(edges), 1, 0, 0)
            call = lambda: ctx._check(ctx.lib.mdb_hist_batch_dev(ctx.handle, ctypes.byref(resident.seg), None,
                                                                 ctypes.byref(request), edges.ctypes.data,
                                                                 ctypes.c_void_p(dev_counts)))
            hist = timed(ctx, call, repeats)
            ctx.dev_free(dev_counts)
            assert int(ctx.hist_dev(resident, edges).sum()) == n_points
            result[f"hist_{n_edges}_edges"] = {"edges": len(edges), "ms": round(hist[0], 4), "kernels": hist[1],
                                              "x_rebuild": round(hist[0] / rebuild[0], 3)}
            print(f"{name:28s} hist {len(edges):4d} edges {hist[0]:9.3f} ms  (rebuild of the values {rebuild[0]:9.3f} ms)",
                  flush=True)
        median = timed(ctx, lambda: ctx.quantile_dev(resident, [0.5]), repeats)
        lo, hi, counted = ctx.quantile_dev(resident, [0.5])
        assert counted == n_points
        result["median"] = {"ms": round(median[0], 4), "kernels": median[1], "passes": median[1].get("k_hist", [0])[0],
                            "x_rebuild": round(median[0] / rebuild[0], 3), "lo": float(lo[0]), "hi": float(hi[0])}
        sixteen = timed(ctx, lambda: ctx.quantile_dev(resident, [k / 15.0 for k in range(16)]), repeats)
        result["sixteen_quantiles"] = {"ms": round(sixteen[0], 4), "passes": sixteen[1].get("k_hist", [0])[0]}
        print(f"{name:28s} median {median[0]:9.3f} ms in {result['median']['passes']} passes; 16 quantiles "
              f"{sixteen[0]:9.3f} ms in {result['sixteen_quantiles']['passes']} passes", flush=True)
    finally:
        ctx.dev_free(out_val)
        resident.free()
    return result


def fitted_batch(ctx, values, n_series, points, eb, interval):
    starts = np.arange(0, points, CHUNK_POINTS, dtype=np.uint64)
    offsets = (np.arange(n_series, dtype=np.uint64)[:, None] * np.uint64(points) + starts[None, :]).reshape(-1)
    offsets = np.concatenate([offsets, np.array([n_series * points], dtype=np.uint64)])
    offsets_dev, first_index_dev = ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, n_series))
    fitted = ctx.compress_chunks_dev(0, values, offsets_dev, len(offsets) - 1, eb, 0, interval, first_index_dev)
    ctx.sync()
    for pointer in (values, offsets_dev, first_index_dev):
        ctx.dev_free(pointer)
    batch = fitted.download()
    fitted.free()
    return batch


def bench_shaped(ctx, a):
    values = ctx.dev_alloc(4 * a.series * a.points)
    ctx.synth_values_dev(values, 0, a.series, a.points, SEED)
    batch = fitted_batch(ctx, values, a.series, a.points, mdb.error_bound("relative", 1.0), 1000)
    return measure(ctx, f"bench {a.series}x{a.points}", batch, a.repeats)


def mixed(ctx, a, bound):
    eb = mdb.error_bound("lossless") if bound == "lossless" else mdb.error_bound("relative", 1.0)
    host_values = np.concatenate([datagen.mixed_series(a.mixed_points, 1000 + s, (1.0, 1.05) if s % 2 else None)[1]
                                  for s in range(a.mixed_series)])
    batch = fitted_batch(ctx, ctx.upload_array(host_values), a.mixed_series, a.mixed_points, eb, 100)
    return measure(ctx, f"mixed {bound} {a.mixed_series}x{a.mixed_points}", batch, a.repeats)


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
