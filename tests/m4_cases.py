"""The oracle of tests/test_gpu_m4.py: ora.grid_batch's points reduced per cell in numpy by the four rules of M4 - a
lexsort per rule on (t, key) with key the totalOrder key of the f32 bits. Timestamps, the bit patterns of the values
and the counts are exact. Nothing here calls the library under test."""

import numpy as np

import oracle_lib as ora
import modelardb_rs_amd as mdb

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
POINTS = (("t_first", "v_first"), ("t_last", "v_last"), ("t_min", "v_min"), ("t_max", "v_max"))


def keys_of(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def point_buckets(timestamps, origin, width):
    """floor((t - origin) / width) per point as int64 where that fits (-1: below bucket 0 or beyond int64)."""
    if len(timestamps) == 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = int(timestamps.min()) - origin, int(timestamps.max()) - origin
    if I64_MIN <= lo and hi <= I64_MAX:
        return (timestamps - np.int64(origin)) // np.int64(width)
    buckets = [(int(t) - origin) // width for t in timestamps]
    return np.array([b if 0 <= b <= I64_MAX else -1 for b in buckets], dtype=np.int64)


def reduce(timestamps, values, cells, n_cells):
    """The four rules over points that carry their cell number."""
    out = mdb.fresh_m4_cells(n_cells)
    if len(cells) == 0:
        return out
    keys = keys_of(values)
    by_time = np.lexsort((keys, timestamps, cells))
    by_low = np.lexsort((timestamps, keys, cells))
    by_high = np.lexsort((timestamps, -keys, cells))
    sorted_cells = cells[by_time]
    starts = np.flatnonzero(np.concatenate([[True], sorted_cells[1:] != sorted_cells[:-1]]))
    ends = np.concatenate([starts[1:], [len(cells)]]) - 1
    hit = sorted_cells[starts]
    out["count"][hit] = ends - starts + 1
    for (t_name, v_name), rows in zip(POINTS, (by_time[starts], by_time[ends], by_low[starts], by_high[starts])):
        out[t_name][hit] = timestamps[rows]
        out[v_name][hit] = values[rows]
    return out


GRIDS = {}


def grid(batch):
    """ora.grid_batch(batch), computed once per batch object."""
    if id(batch) not in GRIDS:
        timestamps, values, rows, _ = ora.grid_batch(batch)
        GRIDS[id(batch)] = (batch, timestamps.astype(np.int64), values.astype(np.float32), rows.astype(np.int64))
    return GRIDS[id(batch)][1:]


def oracle(batch, groups, n_groups, origin, width, n_buckets, t_lo=I64_MIN, t_hi=I64_MAX):
    timestamps, values, rows = grid(batch)
    groups = np.zeros(len(batch), dtype=np.uint32) if groups is None else groups
    point_groups = np.repeat(groups.astype(np.int64), rows)
    buckets = point_buckets(timestamps, origin, width)
    keep = (timestamps >= t_lo) & (timestamps <= t_hi) & (buckets >= 0) & (buckets < n_buckets)
    cells = point_groups[keep] * n_buckets + buckets[keep]
    return reduce(timestamps[keep], values[keep], cells, n_groups * n_buckets).reshape(n_groups, n_buckets)


def assert_cells(got, expected, context=""):
    """Every member exact (values by bit pattern); the members of an empty cell are not compared beyond its bytes
    being the fresh ones in `expected`."""
    assert got.shape == expected.shape, context
    np.testing.assert_array_equal(got["count"], expected["count"], err_msg=context)
    for t_name, v_name in POINTS:
        np.testing.assert_array_equal(got[t_name], expected[t_name], err_msg=f"{context} {t_name}")
        np.testing.assert_array_equal(got[v_name].view(np.uint32), expected[v_name].view(np.uint32),
                                      err_msg=f"{context} {v_name}")
