"""Cases and the point-by-point reference of the query operators' randomised differential soak (a helper module:
tests/test_gpu_query_soak.py runs the cases on the GPU, tests/test_query_soak_cpu.py keeps this file honest).

make_case(index) sends the input domain of tests/test_gpu_soak.py - value levels from 1e-38 to 3e37 with NaN, infinities,
zeros and subnormals injected, epoch-scale and negative timestamps, intervals of 1 and 60 000 000, gaps up to 2^41,
random error bounds and chunk cuts - through one to four series of one batch, each its own group, with two or three
bucket requests, a value filter, a list of histogram edges and a list of quantiles. reference(case) puts the points of
ora.grid_batch into cells and reduces them with the oracles the operators' own tests use (tests/test_gpu_m4.py,
test_gpu_moments.py, test_gpu_hist.py, test_gpu_hist_buckets.py, test_gpu_agg_buckets_filter.py); the aggregates'
SUM is math.fsum of the cell's points, and is held to

    |got - expected| <= 1e-5 * |expected| + 1e-6 * sum(|v|)     (no absolute floor)

MIN and MAX are compared by bit pattern. One thing is left open, as in test_gpu_agg_buckets_filter._assert_cells: in a
cell that holds both +0.0 and -0.0 and whose extreme is zero, which zero is reported depends on the order the points
are folded in (min_num keeps the first), in the reference's plan as here. The extremes start at +-FLT_MAX
(model_simple_aggregates.rs), so MIN of a cell of +inf alone is FLT_MAX: the identity between M4's v_min / v_max and the
aggregates' MIN / MAX is asked wherever the cell holds no NaN, no infinity and not both zeros."""

import contextlib
import io
import math
import pickle
from types import SimpleNamespace

import numpy as np

import oracle_lib as ora
import modelardb_rs_amd as mdb
import test_gpu_agg_buckets_filter as bucket_filter
import test_gpu_hist as hist
import test_gpu_hist_buckets as hist_buckets
import test_gpu_m4 as m4
import test_gpu_moments as moments
import test_gpu_soak as soak

SEED = 0x51554552
LENGTHS = (1, 2, 9, 60, 700, 5_000, 20_000)
MAX_CELLS = 2048
STYLES = ("cover", "window", "clipped")
Q_LISTS = hist_buckets.Q_LISTS
F32_MAX = np.float32(np.finfo(np.float32).max)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SUM_RELATIVE, SUM_OF_MAGNITUDES = 1e-5, 1e-6   # the two terms of test_gpu_agg_buckets._assert_cells


# ---- the generator ---------------------------------------------------------------------------------------------------

def _neighbour(rng, pool):
    """A value of `pool` or one of its two f32 neighbours."""
    value = np.float32(pool[int(rng.integers(0, len(pool)))])
    step = int(rng.choice([-1, 0, 0, 1]))
    with np.errstate(over="ignore"):
        return value if step == 0 else np.nextafter(value, np.float32(np.inf if step > 0 else -np.inf))


def _cover(rng, first, last):
    span = last - first + 1
    width = -(-span // int(rng.choice([1, 2, 37, 500])))
    origin = first - int(rng.integers(0, width))
    return origin, width, (last - origin) // width + 1


def _requests(rng, timestamps):
    first, last = int(timestamps.min()), int(timestamps.max())
    gaps = np.diff(np.sort(timestamps))
    gaps = gaps[gaps > 0]
    delta = max(int(np.median(gaps)), 1) if len(gaps) else 1
    pick = lambda: int(timestamps[int(rng.integers(0, len(timestamps)))])
    requests = []
    for _ in range(int(rng.integers(2, 4))):
        style = STYLES[int(rng.integers(0, 3))]
        t_lo = t_hi = None
        if style == "window":
            origin = pick() + int(rng.integers(-3, 4))
            width = int(rng.choice([1, delta, 7 * delta, 1000 * delta]))
            n_buckets = int(rng.choice([1, 3, 200]))
        else:
            origin, width, n_buckets = _cover(rng, first, last)
            if style == "clipped":
                a, b = sorted((pick(), pick()))
                t_lo, t_hi = a + int(rng.integers(-1, 2)), b + int(rng.integers(-1, 2))
                t_hi = max(t_lo, t_hi)
        requests.append(SimpleNamespace(style=style, origin=origin, width=width, n_buckets=n_buckets, t_lo=t_lo, t_hi=t_hi))
    return requests


def _filter_spec(rng, pool, timestamps):
    """The keyword arguments of mdb.value_filter: about one in ten passes nothing, one in ten everything."""
    kind = rng.random()
    spec = {}
    if kind < 0.1:
        bound = float(_neighbour(rng, pool))
        spec = dict(lo=bound, hi=bound, hi_open=True)
    elif kind >= 0.2:
        lo, hi = sorted((float(_neighbour(rng, pool)), float(_neighbour(rng, pool))))
        ends = rng.choice([0, 1, 1, 2], 2)   # open, closed, absent
        if ends[0] < 2:
            spec.update(lo=lo, lo_open=bool(ends[0] == 0))
        if ends[1] < 2:
            spec.update(hi=hi, hi_open=bool(ends[1] == 0))
    if rng.random() < 0.25:   # the filter's own time range, ANDed with the request's
        a, b = sorted(int(timestamps[int(k)]) for k in rng.integers(0, len(timestamps), 2))
        spec.update(t_lo=a, t_hi=b)
    return spec


def _hostile_stretch(rng, values):
    """What the operators' binary searches and tie rules meet nowhere else, written over a stretch of a series in two
    cases out of five: both zeros side by side; a line whose rise per point is far below one ulp of its level (plateaus
    of equal f32 roundings); a line through zero (keys that straddle +-0); a steep line."""
    kind = int(rng.integers(0, 10))
    if kind > 3:
        return values
    n = len(values)
    at = int(rng.integers(0, n))
    length = int(min(n - at, rng.choice([2, 9, 300, 4000])))
    i = np.arange(length, dtype=np.float64)
    if kind == 0:
        values[at:at + length] = np.where(i % 2 == 0, np.float32(0.0), np.float32(-0.0))
    elif kind == 1:
        level = float(values[at]) if np.isfinite(values[at]) and values[at] != 0 else 100.0
        values[at:at + length] = (level * (1.0 + i * float(rng.choice([-1.0, 1.0])) * 2.0 ** -29)).astype(np.float32)
    elif kind == 3:   # (steep: at epoch timestamps one microsecond apart slope * t cancels against the intercept)
        level = float(values[at]) if np.isfinite(values[at]) and abs(values[at]) < 1e30 else 1e-38
        values[at:at + length] = (level * (1.0 + i * float(rng.choice([-3e-3, 1e-4, 3e-3])))).astype(np.float32)
    else:
        scale = float(rng.choice([1e-38, 1e-3, 1.0, 2500.0]))
        values[at:at + length] = (scale * (i - float(rng.integers(0, length))) / length).astype(np.float32)
    return values


def _searched_lines(batch, timestamps, values, rows):
    """(first point, points) of every Swing segment of three or more finite points with regular timestamps."""
    starts = np.concatenate([[0], np.cumsum(rows.astype(np.int64))])
    out = []
    for row in np.flatnonzero((batch.model_type_id == mdb.MDB_SWING_ID) & (rows >= 3)):
        steps = np.diff(timestamps[starts[row]:starts[row + 1]])
        if (steps == steps[0]).all() and np.isfinite(values[starts[row]:starts[row + 1]]).all():
            out.append((int(starts[row]), int(rows[row])))
    return out


def make_case(index):
    """Everything one run needs, a pure function of `index`."""
    rng = np.random.default_rng([SEED, index])
    n_series = int(rng.integers(1, 5))
    parts, kinds, largest_gap, start = [], [], 0, None
    for k in range(n_series):
        n = max(1, int(int(rng.choice(LENGTHS)) * rng.uniform(0.5, 1.0)))
        timestamps, values, eb = soak.random_timestamps(rng, n), soak.random_values(rng, n), soak.random_error_bound(rng)
        values = _hostile_stretch(rng, values)
        steps = np.diff(timestamps)
        kind = "regular" if len(steps) < 2 or (steps == steps[0]).all() else "irregular"
        if rng.random() < 1.0 / 3.0:
            timestamps, kind = soak.gap_shaped_timestamps(4 * index + k, n), "gaps"
        elif rng.random() < 0.15:   # (the regime of test_gpu_soak's case 506: a model that lasts microseconds at epoch scale)
            timestamps, kind = 1658671178037000 + np.arange(n, dtype=np.int64), "regular"
        start = int(timestamps[0]) if start is None else start
        timestamps = timestamps - timestamps[0] + start   # one origin for the series of a case: their buckets overlap
        largest_gap = max(largest_gap, int(np.diff(timestamps).max(initial=0)))
        cuts = np.sort(rng.integers(0, n + 1, int(rng.integers(1, 4))))
        offsets = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
        parts.append(ora.compress_chunks(timestamps, values, offsets, eb))
        kinds.append(kind)
    batch = mdb.SegmentBatch.concat(parts)
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    permuted = bool(rng.random() < 0.5)
    if permuted:   # the sort path: keys fall out of order
        order = rng.permutation(len(batch))
        batch, groups = batch.take(order), groups[order]

    timestamps, values, rows, _ = ora.grid_batch(batch)
    timestamps, values = timestamps.astype(np.int64), values.astype(np.float32)
    segment = np.repeat(np.arange(len(batch)), rows.astype(np.int64))
    finite = values[np.isfinite(values)]
    pool = finite if len(finite) else np.zeros(1, dtype=np.float32)
    # (bounds on the points of Swing segments, where the filters and the histograms search: most of such cases)
    on_lines = np.isfinite(values) & (batch.model_type_id == mdb.MDB_SWING_ID)[segment]
    bound_pool = values[on_lines] if on_lines.any() and rng.random() < 0.7 else pool

    requests = _requests(rng, timestamps)
    assert all(n_series * request.n_buckets <= MAX_CELLS for request in requests)
    filter_spec = _filter_spec(rng, bound_pool, timestamps)
    lines = _searched_lines(batch, timestamps, values, rows)
    if len(lines) and rng.random() < 0.8:
        # both closed bounds ON inner points of Swing segments with regular timestamps: the interval of passing points
        # then ends inside a line, where each of model_run's four binary searches decides one point
        on_points = []
        for _ in range(2):
            start, length = lines[int(rng.integers(0, len(lines)))]
            on_points.append(float(values[start + int(rng.integers(1, length - 1))]))
        kept = {name: filter_spec[name] for name in ("t_lo", "t_hi") if name in filter_spec}
        filter_spec = dict(kept, lo=min(on_points), hi=max(on_points))
    drawn = np.array([_neighbour(rng, bound_pool if rng.random() < 0.5 else pool) if rng.random() < 0.85 else np.float32(rng.choice([0.0, -0.0]))
                      for _ in range(int(rng.integers(1, 65)))], dtype=np.float32)
    edges = hist._floats_of_keys(np.unique(hist._keys(drawn)))   # (sorted in totalOrder, no edge twice: _edge_lists)
    q = list(Q_LISTS[int(rng.integers(0, len(Q_LISTS)))])
    interpolate = bool(rng.random() < 0.5)
    time_range = (None, None)
    if rng.random() < 0.5:
        a, b = sorted(int(timestamps[int(k)]) for k in rng.integers(0, len(timestamps), 2))
        time_range = (a - int(rng.integers(0, 2)), b + int(rng.integers(0, 2)))
    list_cuts = None
    if rng.random() < 0.25:
        list_cuts = [int(c) for c in np.sort(rng.integers(0, len(batch) + 1, int(rng.integers(1, 5))))]
    slice_pairs = bool(rng.random() < 0.25)
    return SimpleNamespace(index=index, batch=batch, groups=groups, n_groups=n_series, kinds=kinds, permuted=permuted,
                           largest_gap=largest_gap, timestamps=timestamps, values=values, segment=segment,
                           requests=requests, filter_spec=filter_spec, edges=edges, q=q, interpolate=interpolate,
                           time_range=time_range, list_cuts=list_cuts, slice_pairs=slice_pairs)


def value_filter(case):
    return mdb.value_filter(**case.filter_spec)


def case_bytes(case):
    """Everything make_case() decided, as bytes."""
    requests = [tuple(sorted(vars(request).items())) for request in case.requests]
    return pickle.dumps((case.batch.rows(), case.groups.tobytes(), case.n_groups, case.kinds, case.permuted,
                         case.timestamps.tobytes(), case.values.tobytes(), requests, sorted(case.filter_spec.items()),
                         case.edges.tobytes(), case.q, case.interpolate, case.time_range, case.list_cuts,
                         case.slice_pairs))


def forget_grids():
    """The oracles keep ora.grid_batch per batch object: dropped when a case is done."""
    for module in (bucket_filter, hist, hist_buckets, m4, moments):
        module._GRIDS.clear()


# ---- the reference ---------------------------------------------------------------------------------------------------

def _time_bounds(t_lo, t_hi):
    return I64_MIN if t_lo is None else t_lo, I64_MAX if t_hi is None else t_hi


def passes(case, flt):
    """Per point: does its value pass the filter's value bounds (totalOrder keys)?"""
    lo, hi = bucket_filter._key_bounds(flt)
    keys = hist._keys(case.values)
    return (keys >= lo) & (keys <= hi)


def place(case, request, keep=None):
    """(kept points, their cell = group * n_buckets + floor((t - origin) / width)) of a request."""
    t_lo, t_hi = _time_bounds(request.t_lo, request.t_hi)
    buckets = m4._point_buckets(case.timestamps, request.origin, request.width)
    inside = (case.timestamps >= t_lo) & (case.timestamps <= t_hi) & (buckets >= 0) & (buckets < request.n_buckets)
    if keep is not None:
        inside &= keep
    return inside, case.groups.astype(np.int64)[case.segment[inside]] * request.n_buckets + buckets[inside]


def reduce_aggregates(values, cells, n_cells):
    """COUNT / MIN / MAX / SUM per cell over points that carry their cell number: the states, the sum of |v| per cell,
    and per cell whether it holds a NaN, an infinity, both zeros."""
    states = mdb.fresh_agg_states(n_cells)
    magnitude = np.zeros(n_cells)
    flags = {name: np.zeros(n_cells, dtype=bool) for name in ("nan", "inf", "zeros")}
    if len(cells) == 0:
        return states, magnitude, flags
    order = np.argsort(cells, kind="stable")
    sorted_cells, sorted_values = cells[order], values[order]
    starts = np.flatnonzero(np.concatenate([[True], sorted_cells[1:] != sorted_cells[:-1]]))
    ends = np.concatenate([starts[1:], [len(cells)]])
    for start, end in zip(starts, ends):
        cell, run = sorted_cells[start], sorted_values[start:end]
        with np.errstate(invalid="ignore"):   # (a signalling NaN)
            wide = run.astype(np.float64)
        numbers = run[~np.isnan(run)]
        if np.isfinite(run).all():
            total = math.fsum(wide)
        else:
            with np.errstate(invalid="ignore"):
                total = float(np.sum(wide))   # (NaN for a NaN or for both infinities, else the infinity)
        states[cell] = (total, end - start, np.min(numbers, initial=F32_MAX), np.max(numbers, initial=-F32_MAX))
        magnitude[cell] = math.fsum(np.abs(wide[np.isfinite(wide)]))
        bits = run.view(np.uint32)
        flags["nan"][cell] = len(numbers) < len(run)
        flags["inf"][cell] = bool(np.isinf(run).any())
        flags["zeros"][cell] = bool((bits == 0).any() and (bits == 0x80000000).any())
    return states, magnitude, flags


def _aggregates(case, request, keep=None):
    inside, cells = place(case, request, keep)
    n_cells = case.n_groups * request.n_buckets
    states, magnitude, flags = reduce_aggregates(case.values[inside], cells, n_cells)
    shape = (case.n_groups, request.n_buckets)
    return SimpleNamespace(states=states.reshape(shape), magnitude=magnitude.reshape(shape),
                           flags={name: flag.reshape(shape) for name, flag in flags.items()})


def _one_cell(values):
    states, magnitude, flags = reduce_aggregates(values, np.zeros(len(values), dtype=np.int64), 1)
    return SimpleNamespace(states=states, magnitude=magnitude, flags=flags)


def interpolated(lo_bits, hi_bits, n_points, q):
    """lo + (hi - lo) * fraction in f64 with p = q * (double)(N - 1), fraction = p - floor(p) (mdb_quantile_positions);
    equal ends are the value itself. lo_bits / hi_bits: (..., len(q)) uint32; n_points: (...)."""
    with np.errstate(invalid="ignore"):   # (a signalling NaN)
        lo, hi = lo_bits.view(np.float32).astype(np.float64), hi_bits.view(np.float32).astype(np.float64)
    last = np.maximum(n_points, 1).astype(np.float64) - 1.0
    positions = np.asarray(q, dtype=np.float64) * last[..., None]
    with np.errstate(invalid="ignore"):
        return np.where(lo_bits == hi_bits, lo, lo + (hi - lo) * (positions - np.floor(positions)))


def request_tuple(request):
    return request.origin, request.width, request.n_buckets, request.t_lo, request.t_hi


def reference(case):
    """What every operator must give for the case: per request and for the whole batch."""
    batch, groups, n_groups = case.batch, case.groups, case.n_groups
    flt = value_filter(case)
    value_passes = passes(case, flt)
    in_filter_range = (case.timestamps >= flt.t_lo) & (case.timestamps <= flt.t_hi)
    out = SimpleNamespace(requests=[], value_passes=value_passes)
    for request in case.requests:
        t_lo, t_hi = _time_bounds(request.t_lo, request.t_hi)
        args = (batch, groups, n_groups, request.origin, request.width, request.n_buckets, t_lo, t_hi)
        lo, hi, n_points, filled = hist_buckets._expected_quantiles(batch, request_tuple(request), case.q, groups, n_groups)
        out.requests.append(SimpleNamespace(
            agg=_aggregates(case, request),
            agg_filter=_aggregates(case, request, value_passes & in_filter_range),
            m4=m4._oracle(*args),
            moments=moments._oracle(*args),
            hist=hist_buckets._expected(batch, case.edges, request_tuple(request), groups, n_groups),
            quantile=SimpleNamespace(lo=lo, hi=hi, n_points=n_points, filled=filled,
                                     interpolated=interpolated(lo, hi, n_points, case.q))))
    # the whole batch: the filtered rows and their aggregate; the histogram and the quantiles under the time range
    keep = value_passes & in_filter_range
    out.filter_rows = (case.timestamps[keep], case.values[keep],
                       np.bincount(case.segment[keep], minlength=len(batch)).astype(np.uint32))
    out.filter_agg = _one_cell(case.values[keep])
    out.mask_bits = value_passes[in_filter_range]
    t_lo, t_hi = _time_bounds(*case.time_range)
    out.hist = hist._expected(batch, case.edges, t_lo, t_hi, groups, n_groups)
    ordered = np.sort(hist._keys(case.values[(case.timestamps >= t_lo) & (case.timestamps <= t_hi)]))
    n = len(ordered)
    positions = [np.float64(x) * np.float64(max(n, 1) - 1) for x in case.q]
    lo = hist._floats_of_keys(ordered[[int(np.floor(p)) for p in positions]] if n else []).view(np.uint32)
    hi = hist._floats_of_keys(ordered[[int(np.ceil(p)) for p in positions]] if n else []).view(np.uint32)
    out.quantile = SimpleNamespace(lo=lo, hi=hi, n_points=n, ordered=ordered,
                                   interpolated=interpolated(lo, hi, np.array(n), case.q) if n else None)
    return out


# ---- the comparison rules: each returns the differences as text, none when the rule holds ---------------------------------

def _where(shape, flat):
    return tuple(int(k) for k in np.unravel_index(flat, shape))


def aggregate_differences(got, expected, exact_zero_sign=False):
    """`got` (AGG_STATE_DTYPE, any shape) against the `expected` of reduce_aggregates, by the rules of this module."""
    want, out = expected.states, []
    if got.shape != want.shape:
        return [f"shape {got.shape} != {want.shape}"]
    for k in np.flatnonzero(got["count"] != want["count"]):
        out.append(f"cell {_where(got.shape, k)} count: got {got['count'].flat[k]}, expected {want['count'].flat[k]}")
    for field in ("min", "max"):
        same = got[field].view(np.uint32) == want[field].view(np.uint32)
        if not exact_zero_sign:
            same |= expected.flags["zeros"] & (got[field] == 0) & (want[field] == 0)
        for k in np.flatnonzero(~same):
            out.append(f"cell {_where(got.shape, k)} {field}: got {got[field].flat[k]!r} "
                       f"({got[field].view(np.uint32).flat[k]:#010x}), expected {want[field].flat[k]!r} "
                       f"({want[field].view(np.uint32).flat[k]:#010x})")
    finite = np.isfinite(want["sum"])
    with np.errstate(invalid="ignore"):
        bad = np.where(finite, ~(np.abs(got["sum"] - want["sum"])
                                 <= SUM_RELATIVE * np.abs(want["sum"]) + SUM_OF_MAGNITUDES * expected.magnitude),
                       ~((got["sum"] == want["sum"]) | (np.isnan(got["sum"]) & np.isnan(want["sum"]))))
    for k in np.flatnonzero(bad):
        out.append(f"cell {_where(got.shape, k)} sum: got {got['sum'].flat[k]!r}, expected {want['sum'].flat[k]!r} "
                   f"(sum of |v| {expected.magnitude.flat[k]!r}, count {want['count'].flat[k]})")
    return out


def state_array(state):
    """An mdb_agg_state of the whole-batch calls as a one-cell array."""
    return np.array([(state.sum, state.count, state.min, state.max)], dtype=mdb.AGG_STATE_DTYPE)


def exact_differences(got, expected, name):
    """Arrays that must be equal by bit pattern (floats as their unsigned integers)."""
    got, expected = np.asarray(got), np.asarray(expected)
    if got.shape != expected.shape:
        return [f"{name}: shape {got.shape} != {expected.shape}"]
    if got.dtype.kind == "f":
        as_bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        same = got.view(as_bits) == np.asarray(expected, dtype=got.dtype).view(as_bits)
    else:
        same = got == expected
    return [f"{name} {_where(got.shape, k)}: got {got.flat[k]!r}, expected {expected.flat[k]!r}"
            for k in np.flatnonzero(~same)]


def m4_differences(got, expected):
    out = []
    for name in expected.dtype.names:
        out += exact_differences(got[name], expected[name], f"cell member {name}")
    return out


def moments_differences(got, expected, context=""):
    """test_gpu_moments._assert_cells, unchanged; its failure as text, with the first cell that misses."""
    try:
        with contextlib.redirect_stdout(io.StringIO()):   # (it prints its figures per call: thousands of lines here)
            moments._assert_cells(got, expected, context)
    except AssertionError as error:
        plain = (expected["count"] > 0) & expected["finite"]
        mean_miss = plain & ~(np.abs(got["mean"] - expected["mean"]) <= moments.MEAN_TOLERANCE * expected["largest"])
        m2_miss = plain & ~(np.abs(got["m2"] - expected["m2"]) <= moments.M2_TOLERANCE * expected["m2"])
        out = [f"test_gpu_moments._assert_cells: {str(error)[:300]}"]
        for name, miss in (("mean", mean_miss), ("m2", m2_miss)):
            for k in np.flatnonzero(miss)[:5]:
                out.append(f"cell {_where(got.shape, k)} {name}: got {got[name].flat[k]!r}, expected "
                           f"{expected[name].flat[k]!r} (count {expected['count'].flat[k]}, largest |v| "
                           f"{expected['largest'].flat[k]!r})")
        return out
    return []


def quantile_differences(lo, hi, n_points, expected):
    out = exact_differences(n_points, expected.n_points, "n_points")
    filled = expected.filled
    out += exact_differences(lo.view(np.uint32)[filled], expected.lo[filled], "lo of filled cell")
    out += exact_differences(hi.view(np.uint32)[filled], expected.hi[filled], "hi of filled cell")
    if not (np.isnan(lo[~filled]).all() and np.isnan(hi[~filled]).all()):
        out.append("a cell without points was written")
    return out


def identity_differences(agg, m4_cells, moments_cells, hist_counts, quantiles, expected, q):
    """The cross-operator identities of one request."""
    out = exact_differences(m4_cells["count"], agg["count"], "m4.count against agg_buckets.count")
    out += exact_differences(moments_cells["count"], agg["count"], "moments.count against agg_buckets.count")
    out += exact_differences(hist_counts.sum(axis=2).astype(np.int64), agg["count"], "hist_buckets cells summed")
    flags = expected.agg.flags
    plain = (agg["count"] > 0) & ~flags["nan"] & ~flags["inf"] & ~flags["zeros"]
    for ours, theirs in (("min", "v_min"), ("max", "v_max")):
        out += exact_differences(m4_cells[theirs][plain], agg[ours][plain], f"m4.{theirs} against agg_buckets.{ours}")
    lo, hi, n_points = quantiles
    filled = n_points > 0
    for x, end, member in ((0.0, lo, "v_min"), (1.0, hi, "v_max")):
        if x in q:   # (M4's lowest / highest point is the smallest / largest totalOrder key)
            out += exact_differences(end[..., q.index(x)][filled], m4_cells[member][filled], f"quantile {x} against m4.{member}")
    return out
