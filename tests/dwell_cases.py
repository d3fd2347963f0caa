"""The reference of tests/test_gpu_dwell*.py: the microseconds per value cell of mdb_dwell_buckets* from the rows of
ora.grid_batch, in Python integers. The linked rule is integral_cases.linked_intervals, applied row by row; on a linked
interval (t0, v0) - (t1, v1) the series holds v0 on [t0, t1); the interval is walked over the buckets it crosses and
each piece e - a is added to the cell of v0 - the number of edges at or below it in totalOrder, tests/hist_buckets_cases'
key function. Everything is exact. Nothing here calls the library under test."""

import bisect

import numpy as np

import hist_buckets_cases as hbc
import integral_cases as ic

I64_MIN, I64_MAX = ic.I64_MIN, ic.I64_MAX
STEP = 1


def cells_of(intervals, edges, n_groups, origin, width, n_buckets):
    """dwell[n_groups][n_buckets][len(edges) + 1] (uint64) of the linked intervals [(t0, v0, t1, v1, group)]."""
    edge_keys = [int(k) for k in hbc.keys_of(edges)]
    assert all(a < b for a, b in zip(edge_keys[:-1], edge_keys[1:])), "edges must ascend in totalOrder"
    n_cells = len(edge_keys) + 1
    dwell = [0] * (n_groups * n_buckets * n_cells)
    last = origin + n_buckets * width   # the end of the last bucket
    if intervals:
        held = hbc.keys_of(np.array([v0 for _, v0, _, _, _ in intervals], dtype=np.float32)).tolist()
    for (t0, _, t1, _, group), key in zip(intervals, held if intervals else []):
        lo, hi = max(t0, origin), min(t1, last)
        if hi <= lo:
            continue
        cell = bisect.bisect_right(edge_keys, key)
        b = (lo - origin) // width
        while b < n_buckets:
            start = origin + b * width
            a, e = max(t0, start), min(t1, start + width)
            if e <= a:
                break
            dwell[(group * n_buckets + b) * n_cells + cell] += e - a
            b += 1
    return np.array(dwell, dtype=np.uint64).reshape(n_groups, n_buckets, n_cells)


def rows_oracle(timestamps, values, edges, n_buckets, origin, width, row_groups=None, n_groups=1, max_gap=None):
    """cells_of over rows given as arrays (values float32: a NaN keeps its sign and payload)."""
    values = np.asarray(values, dtype=np.float32)
    row_groups = [0] * len(values) if row_groups is None else row_groups
    ts = [int(t) for t in timestamps]
    intervals = []
    for r in range(len(ts) - 1):
        if row_groups[r + 1] != row_groups[r] or ts[r + 1] <= ts[r]:
            continue
        if max_gap is not None and ts[r + 1] - ts[r] > max_gap:
            continue
        intervals.append((ts[r], values[r], ts[r + 1], values[r + 1], int(row_groups[r])))
    return cells_of(intervals, edges, n_groups, origin, width, n_buckets)


def oracle(field, edges, groups, n_groups, origin, width, n_buckets, max_gap=None):
    """The reference of a comoments_cases.Field (its linked intervals are kept with the field)."""
    return cells_of(ic.field_intervals(field, groups, max_gap), edges, n_groups, origin, width, n_buckets)


def edges_through(values, n_edges):
    """n_edges distinct float32 edges spread evenly over the totalOrder keys of the finite `values`, ascending."""
    keys = hbc.keys_of(values[np.isfinite(values)])
    lo, hi = int(keys.min()), int(keys.max())
    picked = np.unique(np.linspace(lo, hi, n_edges + 2)[1:-1].astype(np.int64))
    return hbc.floats_of_keys(picked)

