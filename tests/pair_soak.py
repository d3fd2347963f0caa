"""Cases and references of the two-field operators' randomised differential soak (a helper module:
tests/test_gpu_pair_soak.py runs the cases on the GPU, tests/test_pair_soak_cpu.py keeps this file honest).

comoments_buckets and binned_buckets pair row r of an x field with row r of a y field. draw(index) builds both fields
from the hostile input domain of tests/test_gpu_soak.py - levels from 1e-38 to 3e37 with NaN, infinities, both zeros
and subnormals, epoch-scale and negative timestamps, intervals of 1 and 60 000 000, gaps up to 2^41, random error bounds
and chunk cuts - with the pieces the other soaks use (test_gpu_soak.random_*, query_soak._hostile_stretch, _requests,
_neighbour), one to four series per case:

  x           as query_soak.make_case builds its batch: every series compressed by ora.compress_chunks under a random
              bound and random chunk cuts, each series a group, the segments permuted in half the cases (binned's sort
              path), under one of linked_soak.GROUPINGS.
  y           the same timestamps per series, compressed on its own under its own bound and its own cuts, kept in series
              order: the segments of the two fields do not coincide, and a permuted x against an ordered y is paired by
              row number as the operators and the oracle pair them (mdb.h checks the row COUNT only). One cut row per
              series of two rows or more is forced into both fields (`common_rows`): the shard tier cuts there.
  kind of y   KINDS: "independent" (another random_values draw), "specials" (NaN and +-inf written at rows where x has
              none), "constant" (one value per series, lossless), "negated" (minus x's reconstructed grid, lossless: y's
              grid is exactly -x's), "self" (y IS the x batch object), "points" (y in single-point segments, for series
              of at most MAX_POINT_ROWS rows).
  a tail      in a third of the cases 2 to 5 single-point segments with equal timestamps behind both fields, as
              linked_soak appends them.
  requests    two or three of query_soak._requests (cover, window, clipped: t_lo and t_hi cut segments in the middle)
              and linked_soak's far, near and dense styles.
  edges       1 to 64, drawn as make_case draws them: from x's own values, mostly points on Swing lines and their f32
              neighbours, +-0.0 among them.
  list cuts   for x and for y at different segment indices, in a quarter of the cases.
  slices      a slice_pairs size of linked_soak.SLICE_PAIRS in a quarter of the cases.

A case of more than linked_soak.MAX_ROWS rows per field is left out (draw returns None).

The references are comoments_cases.oracle and binned_cases.oracle on two Field-like objects made of ora.grid_batch.
rule_cells / rule_binned are NOT a second reference: they emulate in plain f64 the rule mdb.h documents under "How"
(runs summed with shifted sums around their first pair, merged in input order by a Python port of the merge rule) and
decide conditioning - a cell is well-conditioned when that emulation meets the operators' own tolerance
(comoments_cases / binned_cases) against the exact reference. An ill-conditioned cell is held on the GPU to its exact
members only: count, finiteness, m2 >= 0. No tolerance is defined here."""

import contextlib
import io
import pickle
from types import SimpleNamespace

import numpy as np

import binned_cases as bc
import cases
import comoments_cases as cc
import linked_soak as ls
import oracle_lib as ora
import query_soak as qs
import test_gpu_hist as hist
import test_gpu_soak as soak
import modelardb_rs_amd as mdb

SEED = 0x50414952
MAX_ROWS = ls.MAX_ROWS
MAX_POINT_ROWS = 200
KINDS = ("independent", "specials", "constant", "negated", "self", "points")
GROUPINGS = ls.GROUPINGS
STYLES = ls.STYLES
TAIL_VALUES = ls.TAIL_VALUES
CONSTANTS = (0.0, -0.0, 1.0, -2.5, 100.0, 1e30, 1e-38, -3e37)
PATHS = ("pmc regular", "swing regular", "model with residual tail", "stream values regular", "model irregular",
         "stream values irregular")
I64_MIN, I64_MAX = qs.I64_MIN, qs.I64_MAX


class Field:
    """What comoments_cases.oracle and binned_cases.oracle read of a field: the batch and the oracle's grid of it."""

    def __init__(self, batch):
        self.batch = batch
        ts, values, rows, _ = ora.grid_batch(batch)
        self.ts, self.values, self.rows = ts.astype(np.int64), values.astype(np.float32), rows.astype(np.int64)
        self.segment = np.repeat(np.arange(len(batch)), self.rows)
        self.starts = np.concatenate([[0], np.cumsum(self.rows)]).astype(np.int64)

    def in_range(self, t_lo, t_hi):
        return (self.ts >= t_lo) & (self.ts <= t_hi)


# ---- the generator ---------------------------------------------------------------------------------------------------

def _offsets(rng, n, common):
    """Random chunk cuts of a series of n rows, the common cut row among them."""
    cuts = rng.integers(0, n + 1, int(rng.integers(1, 4))).tolist() + ([] if common is None else [common])
    return np.concatenate([[0], np.sort(cuts), [n]]).astype(np.uint64)


def _y_values(rng, kind, n, x_raw, x_grid):
    """(values, error bound) of one series of y."""
    if kind == "constant":
        return np.full(n, np.float32(CONSTANTS[int(rng.integers(0, len(CONSTANTS)))])), cases.LOSSLESS
    if kind == "negated":
        return -x_grid, cases.LOSSLESS
    values = qs._hostile_stretch(rng, soak.random_values(rng, n))
    if kind == "specials":
        free = np.flatnonzero(np.isfinite(x_raw))
        for at in (free[rng.integers(0, len(free), int(rng.integers(1, 6)))] if len(free) else []):
            values[at] = np.float32([np.nan, np.inf, -np.inf][int(rng.integers(0, 3))])
    return values, soak.random_error_bound(rng)


def _bucket_request(style, origin, width, n_buckets, t_lo=None, t_hi=None):
    return SimpleNamespace(style=style, origin=int(origin), width=int(width), n_buckets=int(n_buckets), t_lo=t_lo, t_hi=t_hi)


def _more_requests(rng, x, row_groups, n_groups):
    """linked_soak's far, near and dense styles over the rows of x (no time range)."""
    timestamps, values = x.ts, x.values
    steps = np.diff(timestamps)
    gaps = steps[(steps > 0) & (row_groups[1:] == row_groups[:-1])]
    gaps = gaps if len(gaps) else steps[steps > 0]
    median_gap = int(np.median(gaps)) if len(gaps) else 1
    first = int(timestamps.min())
    out = []
    width = int(ls.FAR_WIDTHS[int(rng.integers(0, len(ls.FAR_WIDTHS)))])
    ahead = int(rng.integers(0, 2))
    origin = max(first - ahead * width - int(rng.integers(-(1 << 20), 1 << 20)), I64_MIN)
    out.append(_bucket_request("far", origin, width, ahead + 2))
    ok = np.isfinite(values)
    calm = np.flatnonzero(ok & np.concatenate([[True], ok[:-1]]) & np.concatenate([ok[1:], [True]]))
    at = int(timestamps[int(calm[int(rng.integers(0, len(calm)))]) if len(calm) else int(rng.integers(0, len(timestamps)))])
    width = int(ls.NEAR_WIDTHS[int(rng.integers(0, len(ls.NEAR_WIDTHS)))])
    out.append(_bucket_request("near", at + int(rng.integers(-1, 2)), width, int(rng.choice([1, 64, qs.MAX_CELLS // 4]))))
    width = max(1, int([3 * median_gap // 2, median_gap + 1, median_gap - 1, 2 * median_gap + 1][int(rng.integers(0, 4))]))
    a, b = ls._longest_finite_stretch(timestamps, values, row_groups)
    origin = int(timestamps[a]) - int(rng.integers(0, width))
    out.append(_bucket_request("dense", origin, width,
                               min(qs.MAX_CELLS // n_groups, (int(timestamps[b]) - origin) // width + 2)))
    return out


def draw(index):
    """Everything the runs of case `index` need, a pure function of `index`; None when a field would have more than
    MAX_ROWS rows."""
    rng = np.random.default_rng([SEED, index])
    n_series = int(rng.integers(1, 5))
    kind = KINDS[int(rng.integers(0, len(KINDS)))]
    lengths = []
    for _ in range(n_series):
        base = int(rng.choice(qs.LENGTHS))
        if base > MAX_ROWS:   # (alone beyond the limit: drawn again once, or more than a third of the cases would go)
            base = int(rng.choice(qs.LENGTHS))
        lengths.append(max(1, int(base * rng.uniform(0.5, 1.0))))
    if sum(lengths) > MAX_ROWS - 5:   # (five rows are the longest tail)
        return None
    x_parts, y_parts, kinds, common_rows, start, first_row = [], [], [], [], None, 0
    for k, n in enumerate(lengths):
        timestamps, values, eb = soak.random_timestamps(rng, n), soak.random_values(rng, n), soak.random_error_bound(rng)
        values = qs._hostile_stretch(rng, values)
        steps = np.diff(timestamps)
        timing = "regular" if len(steps) < 2 or (steps == steps[0]).all() else "irregular"
        if rng.random() < 1.0 / 3.0:
            timestamps, timing = soak.gap_shaped_timestamps(4 * index + k, n), "gaps"
        elif rng.random() < 0.15:
            timestamps, timing = 1658671178037000 + np.arange(n, dtype=np.int64), "regular"
        start = int(timestamps[0]) if start is None else start
        timestamps = timestamps - timestamps[0] + start
        common = int(rng.integers(1, n)) if n >= 2 else None
        x_part = ora.compress_chunks(timestamps, values, _offsets(rng, n, common), eb)
        x_parts.append(x_part)
        kinds.append(timing)
        common_rows.append(None if common is None else first_row + common)
        first_row += n
        if kind == "self":
            continue
        y_values, y_eb = _y_values(rng, kind, n, values, ora.grid_batch(x_part)[1].astype(np.float32))
        if kind == "points" and n <= MAX_POINT_ROWS:
            y_parts.append(mdb.SegmentBatch.concat([ls._single_point(t, v) for t, v in zip(timestamps, y_values)]))
        else:
            y_parts.append(ora.compress_chunks(timestamps, y_values, _offsets(rng, n, common), y_eb))

    x_batch = mdb.SegmentBatch.concat(x_parts)
    x_series = np.concatenate([np.full(len(part), k, dtype=np.int64) for k, part in enumerate(x_parts)])
    permuted = bool(rng.random() < 0.5)
    if permuted:
        order = rng.permutation(len(x_batch))
        x_batch, x_series = x_batch.take(order), x_series[order]
    y_batch = x_batch if kind == "self" else mdb.SegmentBatch.concat(y_parts)
    y_series = x_series if kind == "self" else np.concatenate([np.full(len(part), k, dtype=np.int64)
                                                               for k, part in enumerate(y_parts)])
    n_groups = n_series
    grouping = GROUPINGS[int(rng.integers(0, len(GROUPINGS)))]
    if grouping == "series":
        groups = x_series.astype(np.uint32)
    elif grouping == "one":
        groups, n_groups = None, 1
    else:
        groups = rng.integers(0, n_groups, len(x_batch)).astype(np.uint32)

    n_tail = 0
    if rng.random() < 1.0 / 3.0:
        n_tail = int(rng.integers(2, 6))
        body = Field(x_batch)
        at = int(body.ts[-1])
        group = 0 if groups is None else int(groups[-1])
        x_tail, y_tail, tail_groups = [], [], []
        for _ in range(n_tail):
            at += int(ls.TAIL_STEPS[int(rng.integers(0, len(ls.TAIL_STEPS)))])
            value = body.values[int(rng.integers(0, len(body.values)))] if rng.random() < 0.5 else \
                np.float32(TAIL_VALUES[int(rng.integers(0, len(TAIL_VALUES)))])
            other = np.float32(TAIL_VALUES[int(rng.integers(0, len(TAIL_VALUES)))])
            if rng.random() >= 2.0 / 3.0:
                group = int(rng.integers(0, n_groups))
            x_tail.append(ls._single_point(at, value))
            y_tail.append(ls._single_point(at, -value if kind == "negated" else other))
            tail_groups.append(group)
        x_batch = mdb.SegmentBatch.concat([x_batch] + x_tail)
        y_batch = x_batch if kind == "self" else mdb.SegmentBatch.concat([y_batch] + y_tail)
        x_series = np.concatenate([x_series, np.full(n_tail, -1, dtype=np.int64)])
        y_series = x_series if kind == "self" else np.concatenate([y_series, np.full(n_tail, -1, dtype=np.int64)])
        if groups is not None:
            groups = np.concatenate([groups, np.array(tail_groups, dtype=np.uint32)])

    x = Field(x_batch)
    y = x if kind == "self" else Field(y_batch)
    assert len(x.ts) == len(y.ts) == sum(lengths) + n_tail <= MAX_ROWS
    row_groups = np.zeros(len(x.ts), dtype=np.int64) if groups is None else groups.astype(np.int64)[x.segment]

    requests = [_bucket_request(r.style, r.origin, r.width, r.n_buckets, r.t_lo, r.t_hi) for r in qs._requests(rng, x.ts)]
    requests += _more_requests(rng, x, row_groups, n_groups)
    for request in requests:   # (query_soak._requests leaves room for four groups; the cap is the same here)
        request.n_buckets = max(1, min(request.n_buckets, qs.MAX_CELLS // n_groups))

    finite = x.values[np.isfinite(x.values)]
    pool = finite if len(finite) else np.zeros(1, dtype=np.float32)
    on_lines = np.isfinite(x.values) & (x.batch.model_type_id == mdb.MDB_SWING_ID)[x.segment]
    bound_pool = x.values[on_lines] if on_lines.any() and rng.random() < 0.7 else pool
    picked = np.array([qs._neighbour(rng, bound_pool if rng.random() < 0.5 else pool) if rng.random() < 0.85
                       else np.float32(rng.choice([0.0, -0.0])) for _ in range(int(rng.integers(1, 65)))], dtype=np.float32)
    edges = hist._floats_of_keys(np.unique(hist._keys(picked)))

    x_cuts = y_cuts = None
    if rng.random() < 0.25:
        x_cuts = [int(c) for c in np.sort(rng.integers(0, len(x_batch) + 1, int(rng.integers(1, 5))))]
        y_cuts = [int(c) for c in np.sort(rng.integers(0, len(y_batch) + 1, int(rng.integers(1, 5))))]
        if y_cuts == x_cuts:   # (at different segment indices)
            y_cuts = [(y_cuts[0] + 1) % (len(y_batch) + 1)] + y_cuts[1:]
            y_cuts.sort()
    slice_pairs = int(ls.SLICE_PAIRS[int(rng.integers(0, len(ls.SLICE_PAIRS)))]) if rng.random() < 0.25 else None
    return SimpleNamespace(index=index, kind=kind, x=x, y=y, groups=groups, n_groups=n_groups, grouping=grouping,
                           n_series=n_series, n_tail=n_tail, kinds=kinds, permuted=permuted, x_series=x_series,
                           y_series=y_series, tail_groups=tail_groups if n_tail else [], row_groups=row_groups,
                           common_rows=common_rows, requests=requests, edges=edges, x_cuts=x_cuts, y_cuts=y_cuts,
                           slice_pairs=slice_pairs)


def case_bytes(drawn):
    """Everything draw() decided, as bytes."""
    requests = [tuple(sorted(vars(request).items())) for request in drawn.requests]
    return pickle.dumps((drawn.kind, drawn.x.batch.rows(), drawn.y.batch.rows(), drawn.y is drawn.x,
                         None if drawn.groups is None else drawn.groups.tobytes(), drawn.n_groups, drawn.grouping,
                         drawn.n_series, drawn.n_tail, drawn.kinds, drawn.permuted, drawn.x_series.tobytes(),
                         drawn.y_series.tobytes(), drawn.tail_groups, drawn.common_rows, requests, drawn.edges.tobytes(),
                         drawn.x_cuts, drawn.y_cuts, drawn.slice_pairs, drawn.x.ts.tobytes(), drawn.x.values.tobytes(),
                         drawn.y.ts.tobytes(), drawn.y.values.tobytes()))


def time_bounds(request):
    return I64_MIN if request.t_lo is None else request.t_lo, I64_MAX if request.t_hi is None else request.t_hi


def window(request):
    """The bucket arguments of the calls, the time range as keywords."""
    return (request.origin, request.width, request.n_buckets), dict(t_lo=request.t_lo, t_hi=request.t_hi)


def slices(drawn):
    """(xs, ys, groups per batch of xs) of the list forms: each field cut at its own segment indices."""
    x_cuts, y_cuts = [0] + drawn.x_cuts + [len(drawn.x.batch)], [0] + drawn.y_cuts + [len(drawn.y.batch)]
    return ([drawn.x.batch.slice(a, b) for a, b in zip(x_cuts[:-1], x_cuts[1:])],
            [drawn.y.batch.slice(a, b) for a, b in zip(y_cuts[:-1], y_cuts[1:])],
            None if drawn.groups is None else [drawn.groups[a:b] for a, b in zip(x_cuts[:-1], x_cuts[1:])])


def y_groups(drawn):
    """The groups of a "series" case per segment of y (the swap: y takes x's place)."""
    assert drawn.grouping == "series"
    return np.concatenate([drawn.y_series[:len(drawn.y.batch) - drawn.n_tail],
                           np.array(drawn.tail_groups, dtype=np.int64)]).astype(np.uint32)


def describe(request):
    return f"{request.style}: origin {request.origin}, width {request.width}, {request.n_buckets} buckets, " \
           f"range [{request.t_lo}, {request.t_hi}]"


# ---- the references: the operators' own, on the two grids -------------------------------------------------------------

def reference_comoments(drawn, request, swapped=False):
    x, y, groups = (drawn.y, drawn.x, y_groups(drawn)) if swapped else (drawn.x, drawn.y, drawn.groups)
    return cc.oracle(x, y, groups, drawn.n_groups, request.origin, request.width, request.n_buckets, *time_bounds(request))


def reference_binned(drawn, request):
    return bc.oracle(drawn.x, drawn.y, drawn.edges, drawn.groups, drawn.n_groups, request.origin, request.width,
                     request.n_buckets, *time_bounds(request))


# ---- the rule of mdb.h in plain f64: what decides conditioning ------------------------------------------------------------

def merge_comoments(a, b):
    """The merge rule of mdb_comoments_merge_n on (count, mean_x, mean_y, m2_x, m2_y, c_xy) tuples of Python floats."""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    na, nb = float(a[0]), float(b[0])
    count = a[0] + b[0]
    n = float(count)
    dx, dy = b[1] - a[1], b[2] - a[2]
    w = na * nb / n
    return (count, a[1] + dx * (nb / n), a[2] + dy * (nb / n), a[3] + b[3] + dx * dx * w, a[4] + b[4] + dy * dy * w,
            a[5] + b[5] + dx * dy * w)


def merge_moments(a, b):
    """The merge rule of mdb_moments_merge_n on (count, mean, m2) tuples of Python floats."""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    na, nb = float(a[0]), float(b[0])
    count = a[0] + b[0]
    n = float(count)
    d = b[1] - a[1]
    return (count, a[1] + d * (nb / n), a[2] + b[2] + d * d * (na * nb / n))


def merged_arrays(into, from_, merge):
    """`merge` applied cell by cell to two structured arrays: a new array of into's dtype."""
    out = into.copy().reshape(-1)
    flat = np.ascontiguousarray(from_).reshape(-1)
    for k in range(out.size):
        merged = merge(tuple(out[k].tolist()), tuple(flat[k].tolist()))
        out[k] = tuple(np.int64(merged[0]) if j == 0 else np.float64(m) for j, m in enumerate(merged))
    return out.reshape(into.shape)


def _kept_pairs(drawn, request, x=None, y=None, groups=None):
    """The pairs a call counts, in input order: (x values, y values, cell = group * n_buckets + bucket, x segment, row)."""
    x, y = drawn.x if x is None else x, drawn.y if y is None else y
    groups = drawn.groups if groups is None else groups
    t_lo, t_hi = time_bounds(request)
    keep_x, keep_y = x.in_range(t_lo, t_hi), y.in_range(t_lo, t_hi)
    ts, xv, yv, segment = x.ts[keep_x], x.values[keep_x], y.values[keep_y], x.segment[keep_x]
    point_groups = np.zeros(len(ts), dtype=np.int64) if groups is None else groups.astype(np.int64)[segment]
    buckets = cc._point_buckets(ts, request.origin, request.width)
    keep = (buckets >= 0) & (buckets < request.n_buckets)
    return xv[keep], yv[keep], point_groups[keep] * request.n_buckets + buckets[keep], segment[keep], np.flatnonzero(keep)


def _run_starts(cells, segment, rows):
    return np.flatnonzero(np.concatenate([[True], (cells[1:] != cells[:-1]) | (segment[1:] != segment[:-1])
                                          | (rows[1:] != rows[:-1] + 1)]))


def _shifted(values, starts):
    """Per run: (n, K, s1, s2 parts) - d = (double)v - K around the run's first value."""
    wide = values.astype(np.float64)
    lengths = np.diff(np.concatenate([starts, [len(wide)]]))
    d = wide - np.repeat(wide[starts], lengths)
    return lengths, wide[starts], d


def rule_cells(drawn, request, swapped=False):
    """comoments cells by the rule of mdb.h under "How" in plain f64: a run is the pairs of one x segment in one bucket,
    summed around its first pair; runs merge in input order. A dict of flat arrays over n_groups * n_buckets cells."""
    args = (drawn.y, drawn.x, y_groups(drawn)) if swapped else (None, None, None)
    xv, yv, cells, segment, rows = _kept_pairs(drawn, request, *args)
    n_cells = drawn.n_groups * request.n_buckets
    out = [(0, 0.0, 0.0, 0.0, 0.0, 0.0)] * n_cells
    if len(cells):
        with np.errstate(all="ignore"):
            starts = _run_starts(cells, segment, rows)
            n, kx, dx = _shifted(xv, starts)
            _, ky, dy = _shifted(yv, starts)
            sx, sy = np.add.reduceat(dx, starts), np.add.reduceat(dy, starts)
            sxx, syy, sxy = np.add.reduceat(dx * dx, starts), np.add.reduceat(dy * dy, starts), np.add.reduceat(dx * dy, starts)
            count = n.astype(np.float64)
            m2_x, m2_y = sxx - sx * sx / count, syy - sy * sy / count
            m2_x, m2_y = np.where(m2_x < 0.0, 0.0, m2_x), np.where(m2_y < 0.0, 0.0, m2_y)
            runs = zip(n.tolist(), (kx + sx / count).tolist(), (ky + sy / count).tolist(), m2_x.tolist(), m2_y.tolist(),
                       (sxy - sx * sy / count).tolist())
            for cell, run in zip(cells[starts].tolist(), runs):
                out[cell] = merge_comoments(out[cell], run)
    columns = list(zip(*out))
    return {name: np.array(column, dtype=np.int64 if name == "count" else np.float64).reshape(drawn.n_groups, request.n_buckets)
            for name, column in zip(("count",) + cc.MEMBERS, columns)}


def rule_binned(drawn, request):
    """binned cells by the rule of mdb.h: a run is a maximal stretch of consecutive pairs of one x segment in one bucket
    and one value cell, summed around its first y; runs merge in input order. Also "keys ascend": do the runs' cell
    numbers never fall in input order (no sort is needed)?"""
    xv, yv, cells, segment, rows = _kept_pairs(drawn, request)
    n_value_cells = len(drawn.edges) + 1
    cells = cells * n_value_cells + bc.cells_of(xv, drawn.edges)
    n_cells = drawn.n_groups * request.n_buckets * n_value_cells
    out = {}
    ascend = True
    if len(cells):
        with np.errstate(all="ignore"):
            starts = _run_starts(cells, segment, rows)
            n, k, d = _shifted(yv, starts)
            s1, s2 = np.add.reduceat(d, starts), np.add.reduceat(d * d, starts)
            count = n.astype(np.float64)
            m2 = s2 - s1 * s1 / count
            m2 = np.where(m2 < 0.0, 0.0, m2)
            keys = cells[starts]
            ascend = bool((keys[1:] >= keys[:-1]).all())
            for cell, run in zip(keys.tolist(), zip(n.tolist(), (k + s1 / count).tolist(), m2.tolist())):
                out[cell] = merge_moments(out.get(cell, (0, 0.0, 0.0)), run)
    shape = (drawn.n_groups, request.n_buckets, n_value_cells)
    result = {"count": np.zeros(n_cells, dtype=np.int64), "mean": np.zeros(n_cells), "m2": np.zeros(n_cells)}
    for cell, (count, mean, m2) in out.items():
        result["count"][cell], result["mean"][cell], result["m2"][cell] = count, mean, m2
    result = {name: array.reshape(shape) for name, array in result.items()}
    result["keys ascend"] = ascend
    return result


def well_conditioned_cells(rule, expected):
    """Per comoments cell of finite points: does the f64 emulation meet comoments_cases' tolerances against the exact
    reference? (Cells without pairs or with a non-finite point: True - nothing numeric is asked of them.)"""
    plain = (expected["count"] > 0) & expected["finite_x"] & expected["finite_y"]
    well = np.ones(plain.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for field in ("x", "y"):
            well &= np.abs(rule["mean_" + field] - expected["mean_" + field]) <= cc.MEAN_TOLERANCE * expected["largest_" + field]
            well &= np.abs(rule["m2_" + field] - expected["m2_" + field]) <= cc.M2_TOLERANCE * expected["m2_" + field]
        scale = np.sqrt(expected["m2_x"] * expected["m2_y"])
        well &= np.abs(rule["c_xy"] - expected["c_xy"]) <= cc.C_TOLERANCE * scale
    return well | ~plain, plain


def well_conditioned_binned(rule, expected):
    plain = (expected["count"] > 0) & expected["finite"]
    with np.errstate(all="ignore"):
        well = (np.abs(rule["mean"] - expected["mean"]) <= bc.MEAN_TOLERANCE * expected["largest"]) & \
               (np.abs(rule["m2"] - expected["m2"]) <= bc.M2_TOLERANCE * expected["m2"])
    return well | ~plain, plain


# ---- the comparison rules: the operators' own assertions, ill-conditioned cells held to their exact members --------------

def _masked(got, expected, well, plain, members, m2_members):
    """(differences of the exact members of the ill-conditioned cells, `got` with those cells' f64 members replaced by
    the reference's)."""
    ill = plain & ~well
    out, masked = [], got.copy()
    for name in members:
        if not np.isfinite(got[name][ill]).all():
            out.append(f"ill-conditioned cell: {name} is not finite")
        masked[name][ill] = expected[name][ill]
    for name in m2_members:
        if not (got[name][ill] >= 0.0).all():
            out.append(f"ill-conditioned cell: {name} < 0")
    return out, masked


def _held(assert_cells, got, expected, context):
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            assert_cells(got, expected, context)
    except AssertionError as error:
        return [f"{assert_cells.__module__}.assert_cells: {str(error)[:600]}"]
    return []


def comoments_differences(got, expected, well, plain, context=""):
    """comoments_cases.assert_cells, unchanged, on every cell; the f64 members of the ill-conditioned ones excused."""
    out, masked = _masked(got, expected, well, plain, cc.MEMBERS, ("m2_x", "m2_y"))
    return out + _held(cc.assert_cells, masked, expected, context)


def binned_differences(got, expected, well, plain, context=""):
    out, masked = _masked(got, expected, well, plain, ("mean", "m2"), ("m2",))
    return out + _held(bc.assert_cells, masked, expected, context)


def worst_ratios(got, expected, well, plain, binned=False):
    """The largest error of each member against its allowed value over the well-conditioned cells of finite points."""
    keep = plain & well
    out = {}
    with np.errstate(all="ignore"):
        if binned:
            out["mean"] = np.abs(got["mean"] - expected["mean"])[keep] / (bc.MEAN_TOLERANCE * expected["largest"][keep])
            out["m2"] = np.abs(got["m2"] - expected["m2"])[keep] / (bc.M2_TOLERANCE * expected["m2"][keep])
        else:
            for field in ("x", "y"):
                out["mean_" + field] = np.abs(got["mean_" + field] - expected["mean_" + field])[keep] / \
                    (cc.MEAN_TOLERANCE * expected["largest_" + field][keep])
                out["m2_" + field] = np.abs(got["m2_" + field] - expected["m2_" + field])[keep] / \
                    (cc.M2_TOLERANCE * expected["m2_" + field][keep])
            out["c_xy"] = np.abs(got["c_xy"] - expected["c_xy"])[keep] / \
                (cc.C_TOLERANCE * np.sqrt(expected["m2_x"] * expected["m2_y"])[keep])
    return {name: float(np.nan_to_num(ratio, nan=0.0, posinf=0.0).max(initial=0.0)) for name, ratio in out.items()}


def folded_binned(cells):
    """The binned cells of every (group, bucket) folded over the value cells with mdb.moments_merge, in cell order."""
    out = mdb.fresh_moments_cells(cells.shape[:2])
    for c in range(cells.shape[2]):
        mdb.moments_merge(out, np.ascontiguousarray(cells[:, :, c]))
    return out


# ---- the census: what a case holds ----------------------------------------------------------------------------------------

def segment_paths(batch):
    """Per segment the way the operators walk it: an index into PATHS."""
    sizes = batch.timestamps.lengths()
    irregular = (sizes > 0) & ((batch.timestamps.views[:, 4] & 128) != 0)
    stream = batch.model_type_id == mdb.MDB_MACAQUE_V_ID
    tail = batch.residuals.lengths() > 0
    pmc = batch.model_type_id == mdb.MDB_PMC_MEAN_ID
    return np.where(stream, np.where(irregular, 5, 3), np.where(irregular, 4, np.where(tail, 2, np.where(pmc, 0, 1))))


def cut_paths(drawn, request):
    """The paths of the x segments that t_lo falls strictly inside: some of the segment's rows lie before t_lo, some at or
    after it."""
    if request.t_lo is None:
        return set()
    x = drawn.x
    before = np.bincount(x.segment[x.ts < request.t_lo], minlength=len(x.batch))
    inside = (before > 0) & (before < x.rows)
    return set(segment_paths(x.batch)[inside].tolist())
