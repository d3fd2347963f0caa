"""Times the two kernels of mdb_roll_cells_dev (k_roll_suffix, k_roll_windows) with mdb_profile_* on the shapes of
MEASUREMENTS.md's section on rolling windows, and mdb_roll_cells (one host thread) on the same arrays:

    moments cells [1000][100 000]      window 60, stride 1 and stride 60      (2.4 GB of cells)
    uint64        [100][100 000][16]   window 60, stride 1
    change cells  [1000][20 000]       window 60, stride 1

Per row: the median, least and largest milliseconds of each kernel over the repetitions (after warm-up calls of the
same shape), the algorithmic bytes - the cells read once by either kernel that runs, S written and read where a window
starts inside a block, the windows written - their share of the HBM peak at the median, and the host's seconds. The
device's windows are compared with the host's before anything is timed. Reads nothing outside the repository; needs a
GPU (no fallback). Usage: python scripts/measure_roll.py [--out FILE] [--repeat N] [--small]"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO_ROOT)

import modelardb_rs_amd as mdb  # noqa: E402

HBM_PEAK = 8.0e12   # bytes per second, the figure MEASUREMENTS.md prices the HBM at


def cells_of(kind, shape, rng):
    """Cells a per-bucket operator could have made: every tenth one empty."""
    n_outer, n_buckets, n_inner = shape
    row = np.zeros((n_buckets, n_inner), dtype=mdb.ROLL_KINDS[kind])
    if kind == mdb.MDB_ROLL_U64:
        row[...] = rng.integers(0, 1 << 40, row.shape, dtype=np.uint64)
    else:
        count = np.where(rng.random(row.shape) < 0.1, 0, rng.integers(1, 600, row.shape))
        row["count"] = count
        if kind == mdb.MDB_ROLL_MOMENTS:
            row["mean"] = np.where(count > 0, 150.0 + rng.normal(0.0, 20.0, row.shape), 0.0)
            row["m2"] = np.where(count > 0, np.abs(rng.normal(0.0, 50.0, row.shape)) * count, 0.0)
        else:
            row["n_fall"] = count // 2
            row["duration"] = count * 1000
            for name in ("rise", "fall", "reset_sum", "max_rise", "max_fall"):
                row[name] = np.where(count > 0, np.abs(rng.normal(0.0, 5.0, row.shape)), 0.0)
    cells = np.empty(shape, dtype=row.dtype)
    for outer in range(n_outer):   # (every column its own rotation of the row: no two columns alike, one draw)
        cells[outer] = np.roll(row, 7 * outer, axis=0)
    return cells


def measure(context, name, kind, shape, window, stride, repeat, warmup=3):
    rng = np.random.default_rng(2090)
    cells = cells_of(kind, shape, rng)
    n_outer, n_buckets, n_inner = shape
    size = cells.dtype.itemsize
    n_windows = mdb.roll_windows(n_buckets, window, stride)
    n_out = n_outer * n_windows * n_inner
    started = time.perf_counter()
    host = mdb.roll_cells(cells, window, stride)
    host_seconds = time.perf_counter() - started
    dev_cells = context.upload_array(cells)
    dev_out = context.dev_alloc(max(n_out * size, 1))
    try:
        context.roll_cells_dev(kind, dev_cells, n_outer, n_buckets, n_inner, window, stride, dev_out, n_out)
        got = context.download_array(dev_out, n_out, cells.dtype)
        if got.tobytes() != host.tobytes():
            raise SystemExit(f"{name}: the device's windows differ from the host's")
        del got, host
        for _ in range(warmup):
            context.roll_cells_dev(kind, dev_cells, n_outer, n_buckets, n_inner, window, stride, dev_out, n_out)
        context.sync()
        context.profile_enable(True)
        times = {"k_roll_suffix": [], "k_roll_windows": []}
        for _ in range(repeat):
            context.profile_reset()
            context.roll_cells_dev(kind, dev_cells, n_outer, n_buckets, n_inner, window, stride, dev_out, n_out)
            context.sync()
            kernels = context.profile()
            for kernel in times:
                if kernel in kernels:
                    times[kernel].append(kernels[kernel][1])
        context.profile_enable(False)
    finally:
        context.dev_free(dev_cells)
        context.dev_free(dev_out)
    in_bytes = cells.nbytes
    suffix_pass = stride % window != 0 and n_buckets > window
    # S is kept where a window starts inside a block: buckets that are multiples of stride and not of window, in the
    # blocks but the last
    blocks = (n_buckets - 1) // window + 1
    starts = np.arange(0, (blocks - 1) * window, stride) if suffix_pass else np.zeros(0, dtype=np.int64)
    kept = int((starts % window != 0).sum()) * n_outer * n_inner * size
    read_in_suffix = (blocks - 1) * window * n_outer * n_inner * size if suffix_pass else 0
    algorithmic = in_bytes + read_in_suffix + 2 * kept + n_out * size
    row = {"name": name, "shape": list(shape), "cell_bytes": size, "window": window, "stride": stride,
           "n_windows": n_windows, "host_seconds_one_thread": round(host_seconds, 3), "algorithmic_bytes": algorithmic,
           "cells_bytes": in_bytes, "suffix_bytes_kept": kept, "windows_bytes": n_out * size}
    total_median = 0.0
    for kernel, values in times.items():
        if values:
            row[kernel + "_ms"] = {"median": round(statistics.median(values), 4), "min": round(min(values), 4),
                                   "max": round(max(values), 4), "n": len(values)}
            total_median += statistics.median(values)
    row["kernels_ms_median"] = round(total_median, 4)
    row["share_of_hbm_peak"] = round(algorithmic / (total_median * 1e-3) / HBM_PEAK, 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    parser.add_argument("--repeat", type=int, default=20)
    parser.add_argument("--small", action="store_true", help="a hundredth of the columns: a rehearsal of the script")
    arguments = parser.parse_args()
    scale = 100 if arguments.small else 1
    context = mdb.Context(0)
    rows = [
        measure(context, "moments stride 1", mdb.MDB_ROLL_MOMENTS, (1000 // scale, 100_000, 1), 60, 1, arguments.repeat),
        measure(context, "moments stride 60", mdb.MDB_ROLL_MOMENTS, (1000 // scale, 100_000, 1), 60, 60, arguments.repeat),
        measure(context, "u64 16 inner", mdb.MDB_ROLL_U64, (max(100 // scale, 1), 100_000, 16), 60, 1, arguments.repeat),
        measure(context, "change", mdb.MDB_ROLL_CHANGE, (1000 // scale, 20_000, 1), 60, 1, arguments.repeat),
    ]
    context.close()
    if arguments.out:
        os.makedirs(os.path.dirname(os.path.abspath(arguments.out)), exist_ok=True)
        with open(arguments.out, "w") as file:
            json.dump({"device": "MI355X", "hbm_peak_bytes_per_second": HBM_PEAK, "rows": rows}, file, indent=1)


if __name__ == "__main__":
    main()
