"""Cases and references of the linked-row operators' randomised differential soak (a helper module:
tests/test_gpu_linked_soak.py runs the cases on the GPU, tests/test_linked_soak_cpu.py keeps this file honest).

integral_buckets, sample_at, change_buckets and episodes are the operators whose answer depends on the relation between
consecutive rows: same group, time moving forward (episodes: not stepping back), gap within max_gap. draw(index) takes
tests/query_soak.py's case `index` - levels from 1e-38 to 3e37 with NaN, infinities, both zeros and subnormals,
epoch-scale and negative timestamps, intervals of 1 and 60 000 000, gaps up to 2^41, random error bounds, chunk cuts and
segment order - and adds what those operators need:

  the size filter   a case of more than MAX_ROWS rows is left out (draw returns None): the references walk rows in
                    Python. Nothing else is ever left out.
  a grouping        "series" (the case's groups), "one" (groups None: every series seam is a backward step inside the
                    group) or "segments" (a random group per segment: groups change in mid-series).
  a tail            one case in four gets 2 to 5 single-point segments behind its last row, at t_last, t_last again,
                    t_last + 1 and t_last - 1 (each relative to the row before it), each in the group of the segment
                    before it or in another one. They are the only source of consecutive rows with EQUAL timestamps,
                    where the operators differ on purpose: episodes continue on "time not stepping back", the other
                    three need t > t_prev.
  max_gap           per request one of: None, 0, 1, INT64_MAX, a positive gap g between consecutive rows of the data,
                    g - 1, g + 1.
  requests          the case's own (their time range dropped: these operators take none), a "far" one (origin down
                    to INT64_MIN, widths 2^41 + 1 ... INT64_MAX: the saturating bucket ends) and a "near" one (origin a
                    microsecond either side of a row with finite neighbours, widths 1, 2, 1 000, 60 000 000) and a
                    "dense" one (as many buckets as the cap of cells allows over the longest stretch of finite linked
                    rows, of a width near the median gap that is no multiple of it: most linked intervals there are
                    cut by a bucket edge); sample_at gets one more, "own_grid": the instants of one regular series'
                    own grid.
  episodes          the case's value filter with its time range under twelve rules, each a max_gap as above, a min_count
                    of 0, 1, 2 or 7 and a min_duration of 0, 0, the median gap or 1 000 of them.
  slices            where the case asks for them: MDB_AGG_BUCKET_SLICE_PAIRS of 1, 7, 64 or 1 000,
                    MDB_FILTER_SLICE_POINTS of 1, 64, 100 or 1 000.

The rows the references see are ora.grid_batch of the final batch. The references are the operators' own
(integral_cases, sample_cases, change_cases, episodes_cases) and the rules their assert_cells / assert_episodes. Nothing
here calls the library under test, apart from building batches the way the existing tables do."""

import contextlib
import io
import pickle
from types import SimpleNamespace

import numpy as np

import cases
import change_cases as chc
import episodes_cases as ec
import integral_cases as ic
import oracle_lib as ora
import query_soak as qs
import sample_cases as sc
import modelardb_rs_amd as mdb

SEED = 0x4C4E4B44
MAX_ROWS = 8192
I64_MIN, I64_MAX = qs.I64_MIN, qs.I64_MAX
GROUPINGS = ("series", "one", "segments")
GAP_CHOICES = ("none", "zero", "one", "max", "g", "g-1", "g+1")
FAR_WIDTHS = ((1 << 41) + 1, (1 << 54) + 3, (1 << 62) + 5, I64_MAX)
NEAR_WIDTHS = (1, 2, 1000, 60_000_000)
STYLES = qs.STYLES + ("far", "near", "dense")
N_EPISODE_RULES = 12
TAIL_STEPS = (0, 0, 1, -1)
TAIL_VALUES = (0.0, -0.0, 1.0, -2.5, 1e30, 1e-38)
SLICE_PAIRS = (1, 7, 64, 1000)
SLICE_POINTS = (1, 64, 100, 1000)
MIN_COUNTS = (0, 1, 2, 7)
INTEGRAL_METHODS = ((ic.LINEAR, "linear"), (ic.STEP, "step"))
SAMPLE_METHODS = sc.METHODS


# ---- the generator ---------------------------------------------------------------------------------------------------

def _single_point(timestamp, value):
    return ora.try_compress_univariate_time_series(np.array([timestamp], dtype=np.int64),
                                                   np.array([value], dtype=np.float32), cases.LOSSLESS)


def _max_gap(rng, gaps):
    """(name of the choice, max_gap)."""
    choice = GAP_CHOICES[int(rng.integers(0, len(GAP_CHOICES)))]
    g = int(gaps[int(rng.integers(0, len(gaps)))])
    return choice, {"none": None, "zero": 0, "one": 1, "max": I64_MAX, "g": g, "g-1": g - 1, "g+1": g + 1}[choice]


def _request(rng, gaps, style, origin, width, n_buckets, **more):
    choice, max_gap = _max_gap(rng, gaps)
    return SimpleNamespace(style=style, origin=int(origin), width=int(width), n_buckets=int(n_buckets), max_gap=max_gap,
                           gap_choice=choice, **more)


def _own_grid(rng, gaps, kinds, series_of_row, timestamps, n_groups):
    """The instants of one regular series' own grid: origin one of its timestamps, width its interval."""
    candidates = [k for k, kind in enumerate(kinds) if kind == "regular"]
    if not candidates:
        return None
    series = candidates[int(rng.integers(0, len(candidates)))]
    own = np.unique(timestamps[series_of_row == series])
    interval = int(np.diff(own).min()) if len(own) > 1 else 1
    origin = int(own[int(rng.integers(0, len(own) // 4 + 1))])
    n_instants = min(qs.MAX_CELLS // n_groups, (int(own[-1]) - origin) // interval + 1 + int(rng.integers(0, 3)))
    return _request(rng, gaps, "own_grid", origin, interval, n_instants, series=series)


def _longest_finite_stretch(timestamps, values, row_groups):
    """(first row, last row) of the longest run of consecutive rows with finite values in which every row follows the
    one before it in the same group at a later time; the first of equally long runs."""
    ok = np.isfinite(values)
    joins = ok[1:] & ok[:-1] & (row_groups[1:] == row_groups[:-1]) & (timestamps[1:] > timestamps[:-1])
    starts = np.flatnonzero(np.concatenate([[True], ~joins]))
    lengths = np.diff(np.concatenate([starts, [len(values)]]))
    longest = int(np.argmax(lengths))
    return int(starts[longest]), int(starts[longest] + lengths[longest] - 1)


def draw(index):
    """Everything the four operators' runs of case `index` need, a pure function of `index`; None when the case has more
    than MAX_ROWS rows."""
    case = qs.make_case(index)
    if len(case.timestamps) > MAX_ROWS:
        return None
    rng = np.random.default_rng([SEED, index])
    batch, n_groups = case.batch, case.n_groups
    series_of_segment = case.groups.astype(np.int64)
    grouping = GROUPINGS[int(rng.integers(0, len(GROUPINGS)))]
    if grouping == "series":
        groups = case.groups.copy()
    elif grouping == "one":
        groups, n_groups = None, 1
    else:
        groups = rng.integers(0, n_groups, len(batch)).astype(np.uint32)

    n_tail = 0
    if rng.random() < 0.25:
        n_tail = int(rng.integers(2, 6))
        at = int(case.timestamps[-1])
        group = 0 if groups is None else int(groups[-1])
        parts, tail_groups = [batch], []
        for _ in range(n_tail):
            at += int(TAIL_STEPS[int(rng.integers(0, len(TAIL_STEPS)))])
            if rng.random() < 0.5:
                value = case.values[int(rng.integers(0, len(case.values)))]
            else:
                value = np.float32(TAIL_VALUES[int(rng.integers(0, len(TAIL_VALUES)))])
            if rng.random() >= 2.0 / 3.0:
                group = int(rng.integers(0, n_groups))
            parts.append(_single_point(at, value))
            tail_groups.append(group)
        assert all(len(part) == 1 for part in parts[1:])
        batch = mdb.SegmentBatch.concat(parts)
        series_of_segment = np.concatenate([series_of_segment, np.full(n_tail, -1, dtype=np.int64)])
        if groups is not None:
            groups = np.concatenate([groups, np.array(tail_groups, dtype=np.uint32)])

    timestamps, values, rows, _ = ora.grid_batch(batch)
    timestamps, values = timestamps.astype(np.int64), values.astype(np.float32)
    segment = np.repeat(np.arange(len(batch)), rows.astype(np.int64))
    assert len(timestamps) == len(case.timestamps) + n_tail
    row_groups = np.zeros(len(timestamps), dtype=np.int64) if groups is None else groups.astype(np.int64)[segment]

    steps = np.diff(timestamps)   # (the domain's timestamps lie within +-2^56: no difference wraps)
    gaps = steps[(steps > 0) & (row_groups[1:] == row_groups[:-1])]
    gaps = gaps if len(gaps) else steps[steps > 0]
    gaps = gaps if len(gaps) else np.ones(1, dtype=np.int64)
    median_gap = int(np.median(gaps))

    first = int(timestamps.min())
    requests = [_request(rng, gaps, r.style, r.origin, r.width, r.n_buckets) for r in case.requests]
    # the origin far below the data (or just inside it): the data in bucket 0 or 1 of very wide buckets, or cut by their edge
    width = int(FAR_WIDTHS[int(rng.integers(0, len(FAR_WIDTHS)))])
    ahead = int(rng.integers(0, 2))
    origin = max(first - ahead * width - int(rng.integers(-(1 << 20), 1 << 20)), I64_MIN)
    requests.append(_request(rng, gaps, "far", origin, width, ahead + 2))
    # the origin a microsecond either side of a timestamp, narrow buckets
    # (beside a row whose neighbours and itself are finite, where there is one: under a wide sampling interval all of
    # these buckets lie inside one link, and a NaN at either end of it would leave nothing in them to compare)
    ok = np.isfinite(values)
    calm = np.flatnonzero(ok & np.concatenate([[True], ok[:-1]]) & np.concatenate([ok[1:], [True]]))
    at = int(timestamps[int(calm[int(rng.integers(0, len(calm)))]) if len(calm) else int(rng.integers(0, len(timestamps)))])
    width = int(NEAR_WIDTHS[int(rng.integers(0, len(NEAR_WIDTHS)))])
    requests.append(_request(rng, gaps, "near", at + int(rng.integers(-1, 2)), width,
                             int(rng.choice([1, 64, qs.MAX_CELLS // 4]))))
    # as many buckets as the cap allows, their width near the median gap and no multiple of it: most links are cut
    width = max(1, int([3 * median_gap // 2, median_gap + 1, median_gap - 1, 2 * median_gap + 1][int(rng.integers(0, 4))]))
    # (over the longest stretch of finite rows that move forward in one group, and no further: the cells of a series
    # that is half NaN only have to be non-finite, and must not carry the test)
    a, b = _longest_finite_stretch(timestamps, values, row_groups)
    origin = int(timestamps[a]) - int(rng.integers(0, width))
    requests.append(_request(rng, gaps, "dense", origin, width,
                             min(qs.MAX_CELLS // n_groups, (int(timestamps[b]) - origin) // width + 2)))
    assert all(n_groups * request.n_buckets <= qs.MAX_CELLS and request.width >= 1 for request in requests)

    sample_requests = list(requests)
    own = _own_grid(rng, gaps, case.kinds, series_of_segment[segment], timestamps, n_groups)
    if own is not None:
        sample_requests.append(own)

    episodes = []
    for _ in range(N_EPISODE_RULES):
        choice, max_gap = _max_gap(rng, gaps)
        episodes.append(SimpleNamespace(max_gap=max_gap, gap_choice=choice,
                                        min_count=int(MIN_COUNTS[int(rng.integers(0, len(MIN_COUNTS)))]),
                                        min_duration=int([0, 0, median_gap, 1000 * median_gap][int(rng.integers(0, 4))])))
    slice_pairs = int(SLICE_PAIRS[int(rng.integers(0, len(SLICE_PAIRS)))])
    slice_points = int(SLICE_POINTS[int(rng.integers(0, len(SLICE_POINTS)))])
    return SimpleNamespace(index=index, batch=batch, groups=groups, n_groups=n_groups, grouping=grouping, n_tail=n_tail,
                           kinds=case.kinds, permuted=case.permuted, timestamps=timestamps, values=values, segment=segment,
                           row_groups=row_groups, series_of_segment=series_of_segment, requests=requests,
                           sample_requests=sample_requests, episodes=episodes, filter_spec=dict(case.filter_spec),
                           slice_pairs=slice_pairs if case.slice_pairs else None,
                           slice_points=slice_points if case.slice_pairs else None, list_cuts=case.list_cuts)


def case_bytes(drawn):
    """Everything draw() decided, as bytes."""
    requests = [tuple(sorted(vars(request).items())) for request in drawn.sample_requests]
    episodes = [tuple(sorted(vars(rule).items())) for rule in drawn.episodes]
    return pickle.dumps((drawn.batch.rows(), None if drawn.groups is None else drawn.groups.tobytes(), drawn.n_groups,
                         drawn.grouping, drawn.n_tail, drawn.kinds, drawn.permuted, drawn.timestamps.tobytes(),
                         drawn.values.tobytes(), drawn.segment.tobytes(), len(drawn.requests), requests,
                         episodes, sorted(drawn.filter_spec.items()), drawn.slice_pairs, drawn.slice_points,
                         drawn.list_cuts))


def value_filter(drawn):
    return mdb.value_filter(**drawn.filter_spec)


def slices(drawn):
    """The batch and its groups cut at the case's rows, for the list forms: links and episodes cross the cuts."""
    cuts = [0] + drawn.list_cuts + [len(drawn.batch)]
    return ([drawn.batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])],
            None if drawn.groups is None else [drawn.groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def describe(request):
    return f"{request.style}: origin {request.origin}, width {request.width}, {request.n_buckets} buckets, " \
           f"max_gap {request.max_gap} ({request.gap_choice})"


# ---- the references: the operators' own, on the rows of the final batch ------------------------------------------------

def linked(drawn, max_gap):
    """integral_cases.linked_intervals of the case under a gap rule, kept with the case."""
    kept = drawn.__dict__.setdefault("_linked", {})
    if max_gap not in kept:
        kept[max_gap] = ic.linked_intervals(drawn.timestamps, drawn.values, drawn.row_groups, max_gap)
    return kept[max_gap]


def reference_integral(drawn, request, method):
    return ic.cells_of(linked(drawn, request.max_gap), drawn.n_groups, request.origin, request.width, request.n_buckets,
                       method)


def reference_sample(drawn, request, method):
    return sc.sample_rows(drawn.timestamps, drawn.values, drawn.row_groups, drawn.n_groups, request.origin, request.width,
                          request.n_buckets, method, request.max_gap)


def reference_change(drawn, request):
    return chc.cells_of(linked(drawn, request.max_gap), drawn.n_groups, request.origin, request.width, request.n_buckets)


def reference_episodes(drawn, rule, min_count=None, min_duration=None):
    """episodes_cases.reference under one of the case's rules (the two minimum filters may be overridden): (episodes, sum
    of magnitudes per episode, n_rows, n_passing, pass bits)."""
    table = SimpleNamespace(batch=drawn.batch, ts=drawn.timestamps, values=drawn.values, segment=drawn.segment)
    return ec.reference(table, value_filter(drawn), drawn.groups, rule.max_gap,
                        rule.min_duration if min_duration is None else min_duration,
                        rule.min_count if min_count is None else min_count)


def own_grid_rows(drawn, request):
    """Of an own_grid request: (the cells that hold exactly one row, the float64 of that row's float32 value per cell)."""
    offsets = drawn.timestamps - np.int64(request.origin)   # (the origin is a timestamp of the data)
    k = offsets // request.width
    on = (offsets >= 0) & (offsets % request.width == 0) & (k < request.n_buckets)
    cells = drawn.row_groups[on] * request.n_buckets + k[on]
    n_cells = drawn.n_groups * request.n_buckets
    rows_in_cell = np.bincount(cells, minlength=n_cells)
    wide = np.zeros(n_cells)
    with np.errstate(invalid="ignore"):   # (a signalling NaN)
        wide[cells] = drawn.values[on].astype(np.float64)
    shape = (drawn.n_groups, request.n_buckets)
    return (rows_in_cell == 1).reshape(shape), wide.reshape(shape)


# ---- the comparison rules: the operators' own assertions, their failure as text -----------------------------------------

def held(assert_cells, got, expected, context):
    """(differences, cells checked numerically, cells that only have to be non-finite) of one of the three assert_cells,
    unchanged."""
    try:
        with contextlib.redirect_stdout(io.StringIO()):   # (each prints its figures per call: thousands of lines here)
            plain, special = assert_cells(got, expected, context)
    except AssertionError as error:
        return [f"{assert_cells.__module__}.assert_cells: {str(error)[:600]}"], 0, 0
    return [], plain, special


def own_grid_differences(drawn, request, got, expected):
    """A series sampled on its own grid is the grid: a cell whose one contribution is a row holds float64(float32 value)
    bit for bit, the sign of a zero and a NaN's payload included. Returns (differences, cells compared)."""
    one_row, wide = own_grid_rows(drawn, request)
    single = one_row & (expected["count"] == 1)
    return qs.exact_differences(got["sum"][single], wide[single], "own-grid cell with count 1"), int(single.sum())


def episodes_differences(got, expected, magnitudes):
    try:
        ec.assert_episodes(got, expected, magnitudes)
    except AssertionError as error:
        return [f"episodes_cases.assert_episodes: {str(error)[:600]}"]
    return []


# ---- the census: what a case holds, counted from the rows and the references ------------------------------------------

def row_census(drawn):
    """Counts over the consecutive rows of one group."""
    t, g, s = drawn.timestamps, drawn.row_groups, drawn.segment
    same = g[1:] == g[:-1]
    return {"seam links": int((same & (t[1:] > t[:-1]) & (s[1:] != s[:-1])).sum()),
            "backward steps": int((same & (t[1:] < t[:-1])).sum()),
            "equal timestamps": int((same & (t[1:] == t[:-1])).sum())}


def edge_crossings(drawn, request):
    """How many linked intervals have pieces in more than one bucket of the request."""
    last = request.origin + request.n_buckets * request.width
    crossing = 0
    for t0, _, t1, _, _ in linked(drawn, request.max_gap):
        lo, hi = max(t0, request.origin), min(t1, last)
        if hi > lo and (hi - 1 - request.origin) // request.width > (lo - request.origin) // request.width:
            crossing += 1
    return crossing


def episodes_over_segments(drawn, episodes):
    """How many of the reference's episodes end in a later segment than they begin."""
    flt = value_filter(drawn)
    segment = drawn.segment[(drawn.timestamps >= flt.t_lo) & (drawn.timestamps <= flt.t_hi)]
    if len(episodes) == 0:
        return 0
    first = episodes["first_row"].astype(np.int64)
    return int((segment[first + episodes["count"].astype(np.int64) - 1] != segment[first]).sum())
