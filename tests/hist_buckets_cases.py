"""The reference of tests/test_gpu_hist_buckets.py: the oracle's grid, every point put into its bucket
(floor((t - origin) / width), inside [0, n_buckets) and [t_lo, t_hi]) and group, then binned with numpy on totalOrder
keys (np.searchsorted(edge_keys, key, side="right")) or sorted by key per (group, bucket). Counts and order statistics
are exact. A request is (origin, width, n_buckets, t_lo, t_hi). Nothing here calls the library under test."""

import numpy as np

import oracle_lib as ora

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

GRIDS = {}


def keys_of(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def floats_of_keys(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return (keys ^ ((keys >> 31) & 0x7FFFFFFF)).astype(np.int32).view(np.float32)


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def grid(batch):
    """(timestamps, values, keys, segment row of every point) of ora.grid_batch, computed once per batch."""
    if id(batch) not in GRIDS:
        timestamps, values, rows, _ = ora.grid_batch(batch)
        segment = np.repeat(np.arange(len(batch)), rows.astype(np.int64))
        GRIDS[id(batch)] = (batch, (timestamps.astype(np.int64), values, keys_of(values), segment))
    return GRIDS[id(batch)][1]


def placed(batch, request, groups):
    """(row = group * n_buckets + bucket, key) of every point the request holds."""
    origin, width, n_buckets, t_lo, t_hi = request
    timestamps, _, keys, segment = grid(batch)
    t_lo, t_hi = I64_MIN if t_lo is None else t_lo, I64_MAX if t_hi is None else t_hi
    keep = (timestamps >= t_lo) & (timestamps <= t_hi) & (timestamps >= origin)
    buckets = (timestamps[keep] - np.int64(origin)) // np.int64(width)
    inside = buckets < n_buckets
    group = np.zeros(int(keep.sum()), dtype=np.int64) if groups is None else groups.astype(np.int64)[segment[keep]]
    return (group * n_buckets + buckets)[inside], keys[keep][inside]


def expected(batch, edges, request, groups=None, n_groups=1):
    rows, keys = placed(batch, request, groups)
    n_buckets, n_cells = request[2], len(edges) + 1
    cells = np.searchsorted(keys_of(edges), keys, side="right")
    counts = np.bincount(rows * n_cells + cells, minlength=n_groups * n_buckets * n_cells)
    return counts.astype(np.uint64).reshape(n_groups, n_buckets, n_cells)


def expected_quantiles(batch, request, q, groups=None, n_groups=1):
    """(lo bits, hi bits, n_points, filled) per (group, bucket) from the sorted cells."""
    rows, keys = placed(batch, request, groups)
    n_rows = n_groups * request[2]
    order = np.lexsort((keys, rows))
    rows, keys = rows[order], keys[order]
    n_points = np.bincount(rows, minlength=n_rows).astype(np.uint64)
    starts = np.concatenate([[0], np.cumsum(n_points.astype(np.int64))[:-1]])
    lo, hi = np.zeros((n_rows, len(q)), dtype=np.uint32), np.zeros((n_rows, len(q)), dtype=np.uint32)
    filled = n_points > 0
    last = n_points[filled].astype(np.float64) - 1.0
    for k, x in enumerate(q):
        p = np.float64(x) * last
        lo[filled, k] = floats_of_keys(keys[starts[filled] + np.floor(p).astype(np.int64)]).view(np.uint32)
        hi[filled, k] = floats_of_keys(keys[starts[filled] + np.ceil(p).astype(np.int64)]).view(np.uint32)
    shape = (n_groups, request[2])
    return lo.reshape(shape + (len(q),)), hi.reshape(shape + (len(q),)), n_points.reshape(shape), filled.reshape(shape)
