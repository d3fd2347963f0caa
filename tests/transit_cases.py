"""The reference of tests/test_gpu_transit*.py: the transitions between value cells of mdb_transit_buckets* from the
rows of ora.grid_batch, in Python integers. The linked rule is integral_cases.linked_intervals, applied row by row; a
linked pair (t0, v0) - (t1, v1) belongs to the bucket of t1 (mdb_change_buckets' rule: never cut, dropped when t1 lies
outside the buckets, t0 anywhere) and adds one to [cell of v0][cell of v1] - a cell being the number of edges at or
below the value in totalOrder, tests/hist_buckets_cases' key function. Everything is exact. Nothing here calls the
library under test."""

import bisect

import numpy as np

import hist_buckets_cases as hbc
import integral_cases as ic

I64_MIN, I64_MAX = ic.I64_MIN, ic.I64_MAX


def cells_of(intervals, edges, n_groups, origin, width, n_buckets):
    """counts[n_groups][n_buckets][n_cells][n_cells] (uint64, [from][to]) of the linked intervals [(t0, v0, t1, v1,
    group)]. Accumulated sparsely: the array may hold millions of counters, the intervals touch few of them."""
    edge_keys = [int(k) for k in hbc.keys_of(edges)]
    assert all(a < b for a, b in zip(edge_keys[:-1], edge_keys[1:])), "edges must ascend in totalOrder"
    n_cells = len(edge_keys) + 1
    sparse = {}
    if intervals:
        before = hbc.keys_of(np.array([v0 for _, v0, _, _, _ in intervals], dtype=np.float32)).tolist()
        after = hbc.keys_of(np.array([v1 for _, _, _, v1, _ in intervals], dtype=np.float32)).tolist()
        for (_, _, t1, _, group), key0, key1 in zip(intervals, before, after):
            if t1 < origin:
                continue
            b = (t1 - origin) // width
            if b >= n_buckets:
                continue
            at = (((group * n_buckets + b) * n_cells + bisect.bisect_right(edge_keys, key0)) * n_cells
                  + bisect.bisect_right(edge_keys, key1))
            sparse[at] = sparse.get(at, 0) + 1
    counts = np.zeros(n_groups * n_buckets * n_cells * n_cells, dtype=np.uint64)
    if sparse:
        counts[np.fromiter(sparse.keys(), dtype=np.int64, count=len(sparse))] = \
            np.fromiter(sparse.values(), dtype=np.uint64, count=len(sparse))
    return counts.reshape(n_groups, n_buckets, n_cells, n_cells)


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


def crossings(counts):
    """(up, down) of mdb_transit_crossings in Python integers: per matrix [from][to] (the last two axes) and edge e,
    up[e] = the sum of counts[from <= e < to], down[e] = the sum of counts[to <= e < from]; uint64, shape (..., n_cells - 1)."""
    counts = np.asarray(counts)
    n_cells = counts.shape[-1]
    flat = counts.reshape(-1, n_cells, n_cells)
    up = np.zeros((flat.shape[0], n_cells - 1), dtype=np.uint64)
    down = np.zeros((flat.shape[0], n_cells - 1), dtype=np.uint64)
    for row, matrix in enumerate(flat):
        for a, b in zip(*np.nonzero(matrix)):
            n = int(matrix[a, b])
            if a < b:
                up[row, a:b] += np.uint64(n)
            elif b < a:
                down[row, b:a] += np.uint64(n)
    shape = counts.shape[:-2] + (n_cells - 1,)
    return up.reshape(shape), down.reshape(shape)
