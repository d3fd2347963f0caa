#!/usr/bin/env python3
"""What does the plan a resident batch keeps save a grid call? In ONE process, so that the box, its clocks and its
memory are the same for both paths: fits a workload on the GPU, makes one call on each path (the second builds the
plan), idles, then times eight blocks of grid_batch_dev calls that alternate MDB_GRID_PLAN_KEEP=0 (the path without a
kept plan: every call plans) and the switch unset (every call runs on the kept plan). A synchronise brackets each
block; the figure is the mean wall time per call. A ninth and a tenth block with the library's profile on give the
HIP-event time of every kernel per call on each path.

The yardstick is the "off" path. The saving per call is set against the summed event time of the kernels that no
longer run: it should reach that sum less the spread (max - min) of the four "off" block means, and every "kept"
block should be faster than its neighbours. Development tool.

  python scripts/profile_grid_plan_keep.py [--workload headline|mixed|all] [--calls 20] [--idle 10]
"""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import modelardb_rs_amd as mdb  # noqa: E402

CHUNK = 65536
SWITCH = b"MDB_GRID_PLAN_KEEP"


def fit_headline(ctx):
    """bench.py's flagship workload: 1 000 series of 10^7 points, relative 1 %."""
    series, points = 1000, 10_000_000
    total = series * points
    values = ctx.dev_alloc(4 * total)
    ctx.synth_values_dev(values, 0, series, points)
    cps = (points + CHUNK - 1) // CHUNK
    offsets = np.array([s * points + c * CHUNK for s in range(series) for c in range(cps)] + [total], dtype=np.uint64)
    first = np.array([c * CHUNK for s in range(series) for c in range(cps)], dtype=np.uint64)
    off_dev, first_dev = ctx.upload_array(offsets), ctx.upload_array(first)
    dev = ctx.compress_chunks_dev(0, values, off_dev, len(offsets) - 1, mdb.error_bound("relative", 1.0), 0, 1000, first_dev)
    for pointer in (values, off_dev, first_dev):
        ctx.dev_free(pointer)
    return dev, total


def mixed_values(ctx):
    """The values of bench.py's mixed_models block at 10^9 points, on the device."""
    import datagen
    points, distinct = 1_000_000, 64
    copies = 1_000_000_000 // (distinct * points)
    series, total = distinct * copies, distinct * copies * points
    host = np.concatenate([datagen.mixed_series(points, 1000 + s, (1.0, 1.05) if s % 2 else None)[1] for s in range(distinct)])
    values = ctx.dev_alloc(4 * total)
    for copy in range(copies):
        ctx.lib.mdb_dev_upload(ctx.handle, values + 4 * copy * distinct * points, host.ctypes.data, host.nbytes)
    starts = np.arange(0, points, CHUNK, dtype=np.uint64)
    offsets = np.concatenate([(s * points + starts) for s in range(series)] + [np.array([total], dtype=np.uint64)]).astype(np.uint64)
    return values, ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, series)), len(offsets) - 1, total


def measure(ctx, label, dev, total, calls, idle):
    out_ts, out_val = ctx.dev_alloc(8 * total), ctx.dev_alloc(4 * total)
    call = lambda: ctx.grid_batch_dev(dev, out_ts, out_val, total)

    def path(kept):
        ctx.lib.mdb_set_option(SWITCH, None if kept else b"0")

    def block(profiled=False):
        ctx.profile_enable(profiled)
        ctx.profile_reset()
        ctx.sync(); started = time.perf_counter()
        for _ in range(calls):
            call()
        ctx.sync(); seconds = time.perf_counter() - started
        kernels = {name: ms / calls for name, (_, ms) in ctx.profile().items()} if profiled else None
        ctx.profile_enable(False)
        return 1e3 * seconds / calls, kernels

    try:
        print(f"== {label}: {len(dev)} segments, {total} points, blocks of {calls} calls, mean wall ms per call", flush=True)
        path(False); call()
        path(True); call()   # (builds the plan)
        time.sleep(idle)
        means = {False: [], True: []}
        order = []
        for k in range(8):
            kept = k % 2 == 1
            path(kept)
            ms, _ = block()
            means[kept].append(ms)
            order.append(ms)
            print(f"block {k + 1} {'kept' if kept else 'off '}: {ms:.3f}", flush=True)
        path(False); _, off_kernels = block(profiled=True)
        path(True); _, kept_kernels = block(profiled=True)
        for name, kernels in (("off ", off_kernels), ("kept", kept_kernels)):
            print(f"block {9 if name == 'off ' else 10} {name}, HIP-event ms per call: " +
                  ", ".join(f"{k} {v:.3f}" for k, v in sorted(kernels.items(), key=lambda kv: -kv[1])), flush=True)
        removed = sum(ms for name, ms in off_kernels.items() if name not in kept_kernels)
        off, kept = means[False], means[True]
        saving, spread = sum(off) / 4 - sum(kept) / 4, max(off) - min(off)
        between = all(order[k] < order[k - 1] and (k + 1 >= len(order) or order[k] < order[k + 1]) for k in range(1, 8, 2))
        print(f"off mean {sum(off) / 4:.3f} (spread {spread:.3f}), kept mean {sum(kept) / 4:.3f} (spread {max(kept) - min(kept):.3f}): "
              f"saving {saving:.3f} ms per call = {100 * saving / (sum(off) / 4):.2f} %")
        print(f"kernels that no longer run, summed event time: {removed:.3f} ms; less the off spread: {removed - spread:.3f} ms; "
              f"saving reaches it: {'yes' if saving >= removed - spread else 'NO'}; every kept block faster than its neighbours: "
              f"{'yes' if between else 'NO'}", flush=True)
    finally:
        ctx.lib.mdb_set_option(SWITCH, None)
        ctx.dev_free(out_ts); ctx.dev_free(out_val)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--workload", choices=("headline", "mixed", "all"), default="all")
    parser.add_argument("--calls", type=int, default=20)
    parser.add_argument("--idle", type=float, default=10.0)
    args = parser.parse_args()
    ctx = mdb.Context(0)
    if args.workload in ("headline", "all"):
        dev, total = fit_headline(ctx)
        measure(ctx, "headline (1 000 series x 10^7 points, relative 1 %)", dev, total, args.calls, args.idle)
        dev.free()
        ctx.trim()
    if args.workload in ("mixed", "all"):
        values, offsets_dev, first_dev, n_chunks, total = mixed_values(ctx)
        for label, eb in (("lossless", mdb.error_bound("lossless")), ("relative 1 %", mdb.error_bound("relative", 1.0))):
            dev = ctx.compress_chunks_dev(0, values, offsets_dev, n_chunks, eb, 0, 100, first_dev)
            measure(ctx, f"mixed models, 10^9 points, {label}", dev, total, args.calls, args.idle)
            dev.free()
    ctx.close()


main()
