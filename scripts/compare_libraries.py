#!/usr/bin/env python3
"""Are two builds of libmdb_hip.so bit-identical on the query operators? Runs one seeded workload once per library, each
in a fresh child process (MDB_HIP_LIBRARY selects the build, _abi.py), prints a SHA-256 digest per call and exits
non-zero if any digest differs. The suite allows SUM a 0.001 % tolerance and so cannot see a reordered addition; this
can: states are compared by their bytes, grids by the bytes of timestamps, values, rows_per_segment and the metrics.

Batches: the bench-shaped and both mixed batches of scripts/profile_value_filter.py, profile_row_mask.py (two fields
each) and profile_bucket_filter.py, at those scripts' default sizes. Per batch: selectivities 0 / 1 / 50 / 100 %, without
a time range and with one that cuts segments; mdb_agg_batch_dev, mdb_agg_batch_range_dev, mdb_agg_batch_filter_dev,
mdb_mask_filter_dev, mdb_agg_batch_mask_dev, mdb_grid_batch_filter_dev, mdb_grid_batch_mask_dev, mdb_agg_buckets_dev,
mdb_agg_buckets_filter_dev and the host forms (mdb_agg_batch, mdb_agg_batch_range, mdb_agg_batch_filter,
mdb_grid_batch_filter_owned, mdb_agg_batch_where, mdb_grid_batch_where_owned, mdb_grid_batch_owned).
Usage (on the GPU box): python3 scripts/compare_libraries.py LIBRARY_A LIBRARY_B [--small]"""
import argparse
from concurrent.futures import ThreadPoolExecutor
import hashlib
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_POINTS = 65536
SEED = 0x4D44425F52454631  # bench.py's
SELECTIVITIES = (0.0, 0.01, 0.50, 1.0)
MINUTE_US = 60_000_000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def child(a):
    import numpy as np
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import modelardb_rs_amd as mdb
    import datagen

    mask_all = mdb.MDB_AGG_COUNT | mdb.MDB_AGG_MIN | mdb.MDB_AGG_MAX | mdb.MDB_AGG_SUM
    ctx = mdb.Context(0)

    pool = ThreadPoolExecutor(8)

    def emit(name, *parts):
        h = hashlib.sha256()
        for part in parts:
            if isinstance(part, np.ndarray):  # (64 MB pieces hashed side by side: hashlib lets go of the interpreter lock)
                raw = np.ascontiguousarray(part).reshape(-1).view(np.uint8)
                pieces = [raw[k:k + (1 << 26)] for k in range(0, len(raw), 1 << 26)]
                for digest in pool.map(lambda piece: hashlib.sha256(piece).digest(), pieces):
                    h.update(digest)
                h.update(str(len(raw)).encode())
            elif part is None:
                h.update(b"<none>")
            else:
                h.update(json.dumps(part, sort_keys=True, default=str).encode())
        print(f"DIGEST\t{h.hexdigest()}\t{name}", flush=True)

    def down(pointer, count, dtype):
        return ctx.download_array(pointer, count, dtype) if count else np.zeros(0, dtype=dtype)

    def state(s):
        return np.frombuffer(struct.pack("<dqff", s.sum, s.count, s.min, s.max), dtype=np.uint8)

    def fit(values, n_series, points, interval, bound):
        starts = np.arange(0, points, CHUNK_POINTS, dtype=np.uint64)
        offsets = (np.arange(n_series, dtype=np.uint64)[:, None] * np.uint64(points) + starts[None, :]).reshape(-1)
        offsets = np.concatenate([offsets, np.array([n_series * points], dtype=np.uint64)])
        offsets_dev, first_index_dev = ctx.upload_array(offsets), ctx.upload_array(np.tile(starts, n_series))
        fitted = ctx.compress_chunks_dev(0, values, offsets_dev, len(offsets) - 1, bound, 0, interval, first_index_dev)
        ctx.sync()
        for pointer in (values, offsets_dev, first_index_dev):
            ctx.dev_free(pointer)
        batch = fitted.download()
        fitted.free()
        return batch, batch.chunk_index.astype(np.int64) // len(starts)

    def bench_field(series, points, seed):
        values = ctx.dev_alloc(4 * series * points)
        ctx.synth_values_dev(values, 0, series, points, seed)
        return fit(values, series, points, 1000, mdb.error_bound("relative", 1.0))

    def mixed_field(series, points, base, bound):
        host = np.concatenate([datagen.mixed_series(points, base + s, (1.0, 1.05) if s % 2 else None)[1] for s in range(series)])
        eb = mdb.error_bound("lossless") if bound == "lossless" else mdb.error_bound("relative", 1.0)
        return fit(ctx.upload_array(host), series, points, 100, eb)

    def filters(resident, n_points, out_ts, out_val, t_lo, t_hi):
        ctx.grid_batch_range_dev(resident, I64_MIN, I64_MAX, out_ts, out_val, n_points)
        step = max(n_points // (1 << 20), 1)
        sample = np.concatenate([ctx.download_array(out_val, min(4096, n_points - k), np.float32, k)
                                 for k in range(0, n_points, step * 4096)])
        sample = np.sort(sample[np.isfinite(sample)])
        out = []
        for s in SELECTIVITIES:
            lo = float(sample[-1]) * 2.0 + 1e30 if s == 0.0 else (-np.inf if s == 1.0 else
                                                                   float(sample[int((1.0 - s) * (len(sample) - 1))]))
            out.append((s, lo, mdb.value_filter(lo=lo, t_lo=t_lo, t_hi=t_hi)))
        return out

    def buckets(name, resident, batch, series_of_segment, t_lo, t_hi, flt):
        first, last = int(batch.start_time.min()), int(batch.end_time.max())
        cells = ctx.agg_buckets_dev(resident, first, MINUTE_US, (last - first) // MINUTE_US + 1,
                                    groups=series_of_segment.astype(np.uint32), t_lo=t_lo, t_hi=t_hi) if flt is None else \
            ctx.agg_buckets_filter_dev(resident, flt, first, MINUTE_US, (last - first) // MINUTE_US + 1,
                                       groups=series_of_segment.astype(np.uint32), t_lo=t_lo, t_hi=t_hi)
        emit(name, cells.view(np.uint8))

    def two_fields(name, field_a, field_b, series_of_segment, host_forms):
        dev_a, dev_b = ctx.upload_segments(field_a), ctx.upload_segments(field_b)
        n_points = ctx.grid_count_range_dev(dev_a, I64_MIN, I64_MAX)
        out_ts, out_val = ctx.dev_alloc(8 * n_points), ctx.dev_alloc(4 * n_points)
        rows = ctx.dev_alloc(4 * max(len(field_a), len(field_b)))
        mask = ctx.dev_alloc(8 * max(mdb.mask_words(n_points), 1))
        first, last = int(field_a.start_time.min()), int(field_a.end_time.max())
        quarter = (last - first) // 4
        emit(f"{name} agg_batch_dev", state(ctx.agg_batch_dev(dev_a, mask_all)))
        if host_forms:
            emit(f"{name} agg_batch", state(ctx.agg_batch(field_a, mask_all)))
            owned = ctx.grid_batch_owned(field_a)
            emit(f"{name} grid_batch_owned", owned[0], owned[1], owned[2], owned[3])
        for range_name, t_lo, t_hi in (("whole", I64_MIN, I64_MAX), ("cut", first + quarter + 123, last - quarter - 77)):
            emit(f"{name} {range_name} agg_batch_range_dev", state(ctx.agg_batch_range_dev(dev_a, t_lo, t_hi, mask_all)))
            buckets(f"{name} {range_name} agg_buckets_dev", dev_a, field_a, series_of_segment, t_lo, t_hi, None)
            if host_forms:
                emit(f"{name} {range_name} agg_batch_range", state(ctx.agg_batch_range(field_a, t_lo, t_hi, mask_all)))
            for s, lo, flt in filters(dev_a, n_points, out_ts, out_val, t_lo, t_hi):
                what = f"{name} {range_name} sel {s:4.2f}"
                emit(f"{what} threshold", lo)
                emit(f"{what} agg_batch_filter_dev", state(ctx.agg_filter_dev(dev_a, flt, mask_all)))
                buckets(f"{what} agg_buckets_filter_dev", dev_a, field_a, series_of_segment, None, None, flt)
                n_out, metrics = ctx.grid_filter_dev(dev_a, flt, out_ts, out_val, n_points, rows)
                emit(f"{what} grid_batch_filter_dev", n_out, metrics, down(out_ts, n_out, np.int64),
                     down(out_val, n_out, np.float32), ctx.download_array(rows, len(field_a), np.uint32))
                n_rows, n_set = ctx.mask_filter_dev(dev_a, flt, mask, mdb.mask_words(n_points))
                emit(f"{what} mask_filter_dev", n_rows, n_set, down(mask, mdb.mask_words(n_rows) * 8, np.uint8))
                emit(f"{what} agg_batch_mask_dev", state(ctx.agg_mask_dev(dev_b, t_lo, t_hi, mask, n_rows, mask_all)))
                n_out, metrics = ctx.grid_mask_dev(dev_b, t_lo, t_hi, mask, n_rows, out_ts, out_val, n_points, rows)
                emit(f"{what} grid_batch_mask_dev", n_out, metrics, down(out_ts, n_out, np.int64),
                     down(out_val, n_out, np.float32), ctx.download_array(rows, len(field_b), np.uint32))
                if host_forms:
                    emit(f"{what} agg_batch_filter", state(ctx.agg_filter(field_a, flt, mask_all)))
                    emit(f"{what} grid_batch_filter_owned", *ctx.grid_filter(field_a, flt, reserve_front=3))
                    emit(f"{what} agg_batch_where", state(ctx.agg_where([field_a], [flt], field_b, mask_all)))
                    emit(f"{what} grid_batch_where_owned", *ctx.grid_where([field_a], [flt], field_b))
                    emit(f"{what} grid_batch_where_owned values", *ctx.grid_where([field_a], [flt], field_b, values_only=True))
        for pointer in (out_ts, out_val, rows, mask):
            ctx.dev_free(pointer)
        dev_a.free()
        dev_b.free()

    def bucket_batch(name, batch, series_of_segment):
        resident = ctx.upload_segments(batch)
        first, last = int(batch.start_time.min()), int(batch.end_time.max())
        quarter = (last - first) // 4
        for range_name, t_lo, t_hi in (("whole", None, None), ("cut", first + quarter + 123, last - quarter - 77)):
            buckets(f"{name} {range_name} agg_buckets_dev", resident, batch, series_of_segment, t_lo, t_hi, None)
            for lo in (-np.inf, 0.0, 1e30):
                flt = mdb.value_filter(lo=lo, t_lo=t_lo, t_hi=t_hi)
                buckets(f"{name} {range_name} lo {lo} agg_buckets_filter_dev", resident, batch, series_of_segment, None, None, flt)
                emit(f"{name} {range_name} lo {lo} agg_batch_filter_dev", state(ctx.agg_filter_dev(resident, flt, mask_all)))
        resident.free()

    shrink = 10 if a.small else 1
    series, points, mixed_points = 10, 10_000_000 // shrink, 1_000_000 // shrink
    (a1, groups), (b1, _) = bench_field(series, points, SEED), bench_field(series, points, SEED + 1)
    two_fields(f"bench {series}x{points}", a1, b1, groups, True)
    for bound in ("lossless", "1%"):
        (a2, groups), (b2, _) = mixed_field(16, mixed_points, 1000, bound), mixed_field(16, mixed_points, 5000, bound)
        two_fields(f"mixed {bound} 16x{mixed_points}", a2, b2, groups, bound == "1%")
    bucket_batch(f"bench {100 // shrink}x{points}", *bench_field(100 // shrink, points, SEED))
    for bound in ("lossless", "1%"):
        bucket_batch(f"mixed {bound} 64x{mixed_points}", *mixed_field(64, mixed_points, 1000, bound))
    ctx.close()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("libraries", nargs="*")
    parser.add_argument("--small", action="store_true", help="a tenth of the points (a quick check of the script)")
    parser.add_argument("--child", action="store_true")
    parser.add_argument("--timeout", type=int, default=500, help="seconds per library")
    a = parser.parse_args()
    if a.child:
        return child(a)
    if len(a.libraries) != 2:
        parser.error("two library paths")
    digests = []
    for library in a.libraries:
        env = dict(os.environ, MDB_HIP_LIBRARY=os.path.abspath(library))
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + (["--small"] if a.small else []), env=env,
                             stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if run.returncode != 0:
            print(f"{library}: the workload failed with status {run.returncode}")
            return 2
        digests.append({line.split("\t")[2]: line.split("\t")[1] for line in run.stdout.splitlines() if line.startswith("DIGEST\t")})
    different = 0
    for name in digests[0]:
        same = digests[0][name] == digests[1].get(name)
        different += not same
        print(f"{'same     ' if same else 'DIFFERENT'} {digests[0][name][:16]} {str(digests[1].get(name))[:16]} {name}")
    different += len(set(digests[1]) - set(digests[0]))
    print(f"{len(digests[0])} calls compared, {different} different")
    return 1 if different or not digests[0] else 0


if __name__ == "__main__":
    sys.exit(main())
