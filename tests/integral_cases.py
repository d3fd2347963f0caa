"""The reference of tests/test_gpu_integral.py: the cells of mdb_integral_buckets* for one field of
tests/comoments_cases.py's tables, from the oracle's grid of the field (Field.ts / Field.values / Field.segment). The
linked rule is applied row by row; every linked interval is walked over the buckets it crosses in Python integers;
the pieces of a cell are summed with math.fsum. Nothing here calls the library under test.

A piece [a, e] of the linked interval (t0, v0) - (t1, v1):
  LINEAR  (e - a) * (v0 + (v1 - v0) * (a + e - 2 t0) / (2 (t1 - t0)))     the trapezoid under the interpolant
  STEP    (e - a) * v0
with the time factors formed from integers (Python's int / int is correctly rounded). The tolerance of a cell is
1e-5 * sum (e - a) * max(|v0|, |v1|) over its pieces, the contract's; the reference's own error is a few 2^-53 of that."""

import math

import numpy as np

import comoments_cases as cc

LINEAR, STEP = 0, 1
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
INTERVAL = cc.INTERVAL
TOLERANCE = 1e-5
AVERAGE_TOLERANCE = 2.0 ** -44   # of |c|, for a cell whose contributing values are all one finite c
CELL_DTYPE = np.dtype([("duration", "<u8"), ("integral", "<f8")])


def linked_intervals(timestamps, values, row_groups, max_gap=None):
    """[(t0, v0, t1, v1, group)] of the consecutive rows that are linked: same group, time moving forward, the gap
    within max_gap (None: no gap rule)."""
    ts = [int(t) for t in timestamps]
    vs = [float(v) for v in values]
    gs = [int(g) for g in row_groups]
    out = []
    for r in range(len(ts) - 1):
        if gs[r + 1] != gs[r] or ts[r + 1] <= ts[r]:
            continue
        if max_gap is not None and ts[r + 1] - ts[r] > max_gap:
            continue
        out.append((ts[r], vs[r], ts[r + 1], vs[r + 1], gs[r]))
    return out


def cells_of(intervals, n_groups, origin, width, n_buckets, method):
    """The cells of the linked intervals: duration (exact), integral (fsum of the pieces; 0.0 where `finite` is False),
    scale (the tolerance's sum), finite (no piece of the cell has a non-finite value that its method reads), pieces
    (how many), and level: the one finite value all pieces of the cell share, else NaN."""
    n_cells = n_groups * n_buckets
    duration = [0] * n_cells
    pieces = [[] for _ in range(n_cells)]
    scales = [[] for _ in range(n_cells)]
    finite = [True] * n_cells
    levels = [set() for _ in range(n_cells)]
    last = origin + n_buckets * width   # the end of the last bucket
    for t0, v0, t1, v1, group in intervals:
        lo, hi = max(t0, origin), min(t1, last)
        if hi <= lo:
            continue
        read_finite = math.isfinite(v0) and (method == STEP or math.isfinite(v1))
        b = (lo - origin) // width
        while b < n_buckets:
            start = origin + b * width
            a, e = max(t0, start), min(t1, start + width)
            if e <= a:
                break
            cell = group * n_buckets + b
            duration[cell] += e - a
            if not read_finite:
                finite[cell] = False
            else:
                if method == STEP or v0 == v1:
                    pieces[cell].append((e - a) * v0)
                    levels[cell].add(v0)
                else:
                    pieces[cell].append((e - a) * (v0 + (v1 - v0) * ((a + e - 2 * t0) / (2 * (t1 - t0)))))
                    levels[cell].add(v0)
                    levels[cell].add(v1)
                scales[cell].append((e - a) * max(abs(v0), abs(v1) if math.isfinite(v1) else abs(v0)))
            b += 1
    shape = (n_groups, n_buckets)
    out = {
        "duration": np.array(duration, dtype=np.uint64).reshape(shape),
        "integral": np.array([math.fsum(p) if ok else 0.0 for p, ok in zip(pieces, finite)]).reshape(shape),
        "scale": np.array([math.fsum(s) for s in scales]).reshape(shape),
        "finite": np.array(finite, dtype=bool).reshape(shape),
        "pieces": np.array([len(p) for p in pieces], dtype=np.int64).reshape(shape),
        "level": np.array([next(iter(l)) if ok and len(l) == 1 else math.nan
                           for l, ok in zip(levels, finite)]).reshape(shape),
    }
    return out


def field_intervals(field, groups, max_gap=None):
    """linked_intervals of a comoments_cases.Field, computed once per (field, grouping, max_gap) and kept with the
    field."""
    cache = field.__dict__.setdefault("_linked_intervals", {})
    key = (None if groups is None else groups.tobytes(), max_gap)
    if key not in cache:
        segment_groups = np.zeros(len(field.batch), dtype=np.uint32) if groups is None else groups
        cache[key] = linked_intervals(field.ts, field.values, segment_groups.astype(np.int64)[field.segment], max_gap)
    return cache[key]


def oracle(field, groups, n_groups, origin, width, n_buckets, method, max_gap=None):
    return cells_of(field_intervals(field, groups, max_gap), n_groups, origin, width, n_buckets, method)


def assert_cells(got, expected, context="", fresh=True):
    """duration equal in every cell; the integral not finite exactly where the reference says so (for a cell with
    pieces) and within TOLERANCE * scale everywhere else. `fresh`: the call began with fresh cells, so a cell without
    a piece is all-zero bytes still. Prints the worst ratio. Returns (plain, special): how many cells of each kind."""
    assert got.shape == expected["duration"].shape, context
    np.testing.assert_array_equal(got["duration"], expected["duration"], err_msg=context)
    hit = expected["duration"] > 0
    if fresh:
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * CELL_DTYPE.itemsize), context
    special = hit & ~expected["finite"]
    plain = hit & expected["finite"]
    assert not np.isfinite(got["integral"][special]).any(), context
    assert np.isfinite(got["integral"][plain]).all(), context
    error = np.abs(got["integral"][plain] - expected["integral"][plain])
    allowed = TOLERANCE * expected["scale"][plain]
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = np.nan_to_num(error / expected["scale"][plain]).max(initial=0.0)
    print(f"{context}: {int(plain.sum())} cells ({int(special.sum())} not finite), integral error / scale <= {worst:.3g} "
          f"(allowed {TOLERANCE:.3g})")
    assert (error <= allowed).all(), context
    return int(plain.sum()), int(special.sum())
