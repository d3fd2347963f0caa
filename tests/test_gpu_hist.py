"""Value histograms and exact quantiles computed on segments (mdb_hist_batch*, mdb_quantile_batch*) against the
reference's plan GridExec -> AggregateExec: the oracle's grid under the time range, binned with numpy on totalOrder keys
(np.searchsorted(edge_keys, key, side="right")) or sorted by key. Counts and order statistics are exact; the host, dev
and list forms and two runs agree byte for byte."""

import ctypes

import numpy as np
import pytest

import cases
import oracle_lib as ora
import scale_cases
import modelardb_rs_amd as mdb

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
PATTERN = 0xA5A5A5A5A5A5A5A5
FIVE_Q = [0.0, 0.25, 0.5, 0.999, 1.0]
SIXTEEN_Q = [k / 15.0 for k in range(16)]


@pytest.fixture(scope="module")
def context():
    ctx = mdb.Context(0)
    yield ctx
    ctx.close()


_GRIDS = {}


def _grid(batch):
    """(timestamps, keys, segment row of every point) of ora.grid_batch, computed once per batch."""
    key = id(batch)
    if key not in _GRIDS:
        timestamps, values, rows, _ = ora.grid_batch(batch)
        segment = np.repeat(np.arange(len(batch)), rows.astype(np.int64))
        _GRIDS[key] = (batch, (timestamps, values, _keys(values), segment))
    return _GRIDS[key][1]


def _keys(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def _floats_of_keys(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return (keys ^ ((keys >> 31) & 0x7FFFFFFF)).astype(np.int32).view(np.float32)


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _bounds(t_lo, t_hi):
    return I64_MIN if t_lo is None else t_lo, I64_MAX if t_hi is None else t_hi


def _expected(batch, edges, t_lo=None, t_hi=None, groups=None, n_groups=1):
    timestamps, _, keys, segment = _grid(batch)
    t_lo, t_hi = _bounds(t_lo, t_hi)
    keep = (timestamps >= t_lo) & (timestamps <= t_hi)
    cells = np.searchsorted(_keys(edges), keys[keep], side="right")
    group = np.zeros(int(keep.sum()), dtype=np.int64) if groups is None else groups.astype(np.int64)[segment[keep]]
    n_cells = len(edges) + 1
    return np.bincount(group * n_cells + cells, minlength=n_groups * n_cells).astype(np.uint64).reshape(n_groups, n_cells)


def _even_edges(keys, n_edges=4095):
    """Up to n_edges edges even in key space strictly between the smallest and the largest key."""
    lo, hi = int(keys.min()), int(keys.max())
    picked = np.unique(np.linspace(lo, hi, n_edges + 2)[1:-1].astype(np.int64))
    picked = picked[(picked > lo) & (picked <= hi)] if hi > lo else np.array([lo], dtype=np.int64)
    return _floats_of_keys(picked)


def _edge_lists(batch):
    """One edge; seven edges ON rebuilt values and on their f32 neighbours; 4 095 edges even in key space between the
    grid's min and max; a list holding -0.0, +0.0, +inf and +NaN."""
    _, values, keys, _ = _grid(batch)
    ordered = np.sort(keys)
    on_values = _floats_of_keys(ordered[[len(ordered) // 5, len(ordered) // 2, (4 * len(ordered)) // 5]])
    with np.errstate(over="ignore", invalid="ignore"):
        around = np.concatenate([np.nextafter(on_values, np.float32(-np.inf)), on_values,
                                 np.nextafter(on_values, np.float32(np.inf))])
    around_keys = np.unique(_keys(around))
    seven = _floats_of_keys(around_keys[:7])
    return {"one": _floats_of_keys(ordered[[len(ordered) // 2]]), "seven": seven, "4095": _even_edges(keys),
            "specials": _f32([0x80000000, 0x00000000, 0x7F800000, 0x7FC00000])}


def _time_ranges(batch):
    """None; the middle half; one that cuts a segment inside its model part; one that cuts a segment inside its
    residual tail (its last point left out; a batch without tails: the model cut again); one without a point."""
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    span = last - first
    lengths = batch.end_time - batch.start_time
    model = batch.model_type_id != mdb.MDB_MACAQUE_V_ID
    longest = int(np.argmax(np.where(model, lengths, -1)))
    model_cut = (int(batch.start_time[longest] + lengths[longest] // 3), last)
    tails = np.flatnonzero(batch.residuals.lengths() > 0)
    tail_cut = (first, int(batch.end_time[tails[len(tails) // 2]]) - 1) if len(tails) else model_cut
    return [(None, None), (first + span // 4, last - span // 4), model_cut, tail_cut, (last + 1, last + 1000)]


def _groupings(n):
    return [(None, 1), (np.arange(n, dtype=np.uint32) % 3, 3), (np.arange(n, dtype=np.uint32) % 3, 5)]


def _check_batch(context, batch, what):
    half = len(batch) // 2
    halves = [batch.slice(0, half), batch.slice(half, len(batch))]
    dev = context.upload_segments(batch)
    try:
        for name, edges in _edge_lists(batch).items():
            for t_lo, t_hi in _time_ranges(batch):
                for groups, n_groups in _groupings(len(batch)):
                    case = (what, name, t_lo, t_hi, n_groups)
                    expected = _expected(batch, edges, t_lo, t_hi, groups, n_groups)
                    host = context.hist(batch, edges, groups, t_lo, t_hi, n_groups=n_groups)
                    assert np.array_equal(host, expected), case
                    on_device = context.hist_dev(dev, edges, groups, t_lo, t_hi, n_groups=n_groups)
                    listed = context.hist_list(halves, edges, None if groups is None else [groups[:half], groups[half:]],
                                               t_lo, t_hi, n_groups=n_groups)
                    again = context.hist(batch, edges, groups, t_lo, t_hi, n_groups=n_groups)
                    assert host.tobytes() == on_device.tobytes() == listed.tobytes() == again.tobytes(), case
                    # a second call ADDS: the counts double, on the host and on the device
                    context.hist(batch, edges, groups, t_lo, t_hi, counts=again)
                    context.hist_dev(dev, edges, groups, t_lo, t_hi, counts=on_device)
                    assert np.array_equal(again, 2 * expected) and np.array_equal(on_device, 2 * expected), case
    finally:
        dev.free()


@pytest.mark.parametrize("irregular", [False, True], ids=["regular", "irregular"])
@pytest.mark.parametrize("eb_name", list(cases.error_bounds()))
def test_mixed_batches_match_the_binned_grid(context, eb_name, irregular):
    _, _, batch = cases.mixed_batch(cases.error_bounds()[eb_name], irregular, seed=1200 + len(eb_name), length=20_000)
    _check_batch(context, batch, (eb_name, irregular))


@pytest.mark.parametrize("eb_name", ["lossless", "abs5"])
def test_edge_cases_nan_inf_and_zeros(context, eb_name):
    _check_batch(context, cases.edge_case_batch(cases.error_bounds()[eb_name]), eb_name)


# ---- the closed form of Swing -------------------------------------------------------------------------------------

def _swing(length, first, last, decreasing=False, start=0, delta=1000):
    return scale_cases.simple_batch([scale_cases.SWING], [start], [length], [delta], [first], [last], [decreasing])


SWING_CASES = {
    "ascending ramp across every cell": lambda: _swing(65_536, 100.0, 200.0),
    "descending ramp across every cell": lambda: _swing(65_536, 100.0, 200.0, decreasing=True),
    "slope 0": lambda: _swing(65_536, 5.0, 5.0),
    "ramp through zero": lambda: _swing(65_536, -5.0, 5.0),
    "ramp down through zero at epoch timestamps": lambda: _swing(30_000, -0.25, 0.5, True, 1_700_000_000_000_000),
    "8 points under 4 095 edges, point by point": lambda: _swing(8, 100.0, 200.0),
    "both ends NaN, point by point": lambda: _swing(16, -np.inf, np.inf),
}


@pytest.mark.parametrize("name", list(SWING_CASES))
def test_swing_segments_in_closed_form(context, name):
    """Single Swing segments on regular timestamps, made with the row builders of tests/scale_cases.py, each under a
    4 095-edge list and a 3-edge list (and edges at -0.0 and +0.0), whole and cut by a time range. The segment whose
    ends rebuild to NaN (a line from -inf to +inf) takes the point-by-point branch of the model part. Its NaNs are
    GENERATED by the arithmetic (inf * 0, inf - inf), and IEEE 754 leaves the sign of such a NaN open: x86, where the
    oracle runs, makes 0xffc00000 and gfx950 makes 0x7fc00000, which totalOrder puts at opposite ends. For that segment
    the oracle's points must equal the rows of grid_batch in everything but that one bit, which is then taken from the
    rows - the points a histogram counts are by definition the rows of mdb_grid_batch_range."""
    batch = SWING_CASES[name]()
    assert batch.model_type_id[0] == mdb.MDB_SWING_ID
    timestamps, values, keys, segment = _grid(batch)
    assert np.isnan(values).all() == ("NaN" in name)
    if "NaN" in name:
        row_timestamps, rows, _, _ = context.grid_batch(batch)
        assert np.array_equal(row_timestamps, timestamps)
        assert np.array_equal(rows.view(np.uint32) & 0x7FFFFFFF, values.view(np.uint32) & 0x7FFFFFFF)
        values, keys = rows, _keys(rows)
        _GRIDS[id(batch)] = (batch, (timestamps, values, keys, segment))
    ordered = np.sort(keys)
    three = _floats_of_keys(np.unique(ordered[[len(ordered) // 4, len(ordered) // 2, (3 * len(ordered)) // 4]]))
    lists = [_even_edges(keys), three, _f32([0x80000000, 0x00000000]), _f32([0x80000000, 0x00000000, 0x3F800000])]
    if "every cell" in name:
        assert len(lists[0]) == 4095
    last = int(batch.end_time[0])
    for edges in lists:
        for t_lo, t_hi in ((None, None), (last // 3 + 1, last - last // 5), (int(batch.start_time[0]) + 1, None)):
            expected = _expected(batch, edges, t_lo, t_hi)
            got = context.hist(batch, edges, None, t_lo, t_hi)
            assert np.array_equal(got, expected), (name, len(edges), t_lo, t_hi)
            if "every cell" in name and t_lo is None and len(edges) == 4095:
                assert np.count_nonzero(expected) > 4000


def test_cells_hold_more_than_32_bits(context):
    """5 000 PMC-Mean segments of 10^6 regular points each (metadata only): every segment is one addition."""
    n, points, delta = 5_000, 1_000_000, 10
    starts = np.arange(n, dtype=np.int64) * points * delta
    batch = scale_cases.simple_batch(np.full(n, scale_cases.PMC), starts, np.full(n, points), np.full(n, delta),
                                     np.full(n, 42.0, dtype=np.float32), np.full(n, 42.0, dtype=np.float32),
                                     np.zeros(n, dtype=bool))
    edges = np.array([41.0, 43.0], dtype=np.float32)
    counts = context.hist(batch, edges)
    assert counts.tolist() == [[0, 5_000_000_000, 0]]
    dev = context.upload_segments(batch)
    try:
        assert context.hist_dev(dev, edges, counts=counts).tolist() == [[0, 10_000_000_000, 0]]
        # a range that cuts the first and the last segment in the middle, three groups
        t_lo, t_hi = int(starts[0]) + 500_000 * delta, int(starts[-1]) + 499_999 * delta
        groups = np.arange(n, dtype=np.uint32) % 3
        per_segment = np.full(n, points, dtype=np.int64)
        per_segment[0] = per_segment[-1] = 500_000
        expected = np.zeros((3, 3), dtype=np.uint64)
        expected[:, 1] = np.bincount(groups, weights=per_segment, minlength=3).astype(np.uint64)
        assert np.array_equal(context.hist_dev(dev, edges, groups, t_lo, t_hi), expected)
        lo, hi, n_points = context.quantile_dev(dev, [0.5])
        assert (lo[0], hi[0], n_points) == (42.0, 42.0, 5_000_000_000)
    finally:
        dev.free()


def test_invariants_against_the_other_operators(context):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["rel1"], True, seed=77, length=20_000)
    edges = _edge_lists(batch)["seven"]
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    dev = context.upload_segments(batch)
    try:
        for t_lo, t_hi in ((first, last), (first + 12_345, last - 23_456)):
            counts = context.hist(batch, edges, groups, t_lo, t_hi, n_groups=3)
            one_bucket = context.agg_buckets(batch, t_lo, t_hi - t_lo + 1, 1, groups=groups, t_lo=t_lo, t_hi=t_hi,
                                             n_groups=3)
            assert counts.sum(axis=1).tolist() == one_bucket["count"][:, 0].tolist()
            assert int(counts.sum()) == context.grid_count_range_dev(dev, t_lo, t_hi)
            whole = counts.sum(axis=0)
            for a in range(len(edges)):
                for b in range(a + 1, len(edges)):
                    flt = mdb.value_filter(lo=float(edges[a]), hi=float(edges[b]), hi_open=True, t_lo=t_lo, t_hi=t_hi)
                    assert int(whole[a + 1:b + 1].sum()) == context.agg_filter(batch, flt, mdb.MDB_AGG_COUNT).count, (a, b)
    finally:
        dev.free()


# ---- errors -------------------------------------------------------------------------------------------------------

def _raw_hist(context, form, batch, dev, groups, dev_groups, request, edges, counts, dev_counts):
    """One raw call of a form ("host", "list", "dev") - the return code; counts / dev_counts receive the result."""
    lib, seg = context.lib, batch.as_c()
    edges_pointer = None if edges is None else edges.ctypes.data_as(ctypes.c_void_p)
    request_pointer = None if request is None else ctypes.byref(request)
    if form == "host":
        return lib.mdb_hist_batch(context.handle, ctypes.byref(seg), None if groups is None else groups.ctypes.data,
                                  request_pointer, edges_pointer, counts.ctypes.data)
    if form == "list":
        pointers = (ctypes.POINTER(mdb._abi.SegmentsC) * 1)(ctypes.pointer(seg))
        group_pointers = (ctypes.c_void_p * 1)(None if groups is None else groups.ctypes.data)
        return lib.mdb_hist_batch_list(context.handle, pointers, group_pointers, 1, request_pointer, edges_pointer,
                                       counts.ctypes.data)
    return lib.mdb_hist_batch_dev(context.handle, ctypes.byref(dev.seg), None if dev_groups is None else
                                  ctypes.c_void_p(dev_groups), request_pointer, edges_pointer, ctypes.c_void_p(dev_counts))


def test_errors_leave_the_counts_untouched(context):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["abs5"], False, seed=5, length=3000)
    n = len(batch)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    good_edges = np.array([120.0, 150.0, 180.0], dtype=np.float32)
    Request = mdb._abi.HistRequestC
    groups = np.arange(n, dtype=np.uint32) % 3
    bad_groups = groups.copy()
    bad_groups[n - 1] = 3  # (the last segment: outside the time range of the request below)
    inside = (first, int(batch.start_time[n - 1]) - 1)
    pattern = np.full(3 * 4, PATTERN, dtype=np.uint64)
    dev = context.upload_segments(batch)
    dev_groups, dev_bad_groups = context.upload_array(groups), context.upload_array(bad_groups)
    dev_counts = context.upload_array(pattern)
    # (request, edges, groups / device groups): every class of error of include/mdb.h
    bad = {
        "flags": (Request(I64_MIN, I64_MAX, 3, 3, 1, 0), good_edges, groups, dev_groups),
        "reserved": (Request(I64_MIN, I64_MAX, 3, 3, 0, 1), good_edges, groups, dev_groups),
        "no edges": (Request(I64_MIN, I64_MAX, 0, 3, 0, 0), good_edges, groups, dev_groups),
        "4096 edges": (Request(I64_MIN, I64_MAX, 4096, 3, 0, 0), np.arange(4096, dtype=np.float32), groups, dev_groups),
        "equal edges": (Request(I64_MIN, I64_MAX, 3, 3, 0, 0), np.array([1, 1, 2], dtype=np.float32), groups, dev_groups),
        "descending edges": (Request(I64_MIN, I64_MAX, 3, 3, 0, 0), np.array([3, 2, 1], dtype=np.float32), groups, dev_groups),
        "-0.0 after +0.0": (Request(I64_MIN, I64_MAX, 3, 3, 0, 0), _f32([0x00000000, 0x80000000, 0x3F800000]), groups,
                            dev_groups),
        "no groups": (Request(I64_MIN, I64_MAX, 3, 0, 0, 0), good_edges, None, None),
        # (2^32 - 1 groups of 4 096 cells: 2^47 bytes of counters)
        "cells that fit no device": (Request(I64_MIN, I64_MAX, 4095, 0xFFFFFFFF, 0, 0), np.arange(4095, dtype=np.float32),
                                     None, None),
        "a group id out of range, outside the time range": (Request(inside[0], inside[1], 3, 3, 0, 0), good_edges,
                                                            bad_groups, dev_bad_groups),
        "NULL request": (None, good_edges, groups, dev_groups),
        "NULL edges": (Request(I64_MIN, I64_MAX, 3, 3, 0, 0), None, groups, dev_groups),
    }
    try:
        for name, (request, edges, host_groups, device_groups) in bad.items():
            for form in ("host", "list", "dev"):
                counts = pattern.copy()
                code = _raw_hist(context, form, batch, dev, host_groups, device_groups, request, edges, counts, dev_counts)
                assert code == 1 and context.lib.mdb_last_error(), (name, form)
                assert np.array_equal(counts, pattern), (name, form)
                assert np.array_equal(context.download_array(dev_counts, len(pattern), np.uint64), pattern), (name, form)
        good = Request(I64_MIN, I64_MAX, 3, 3, 0, 0)
        assert context.lib.mdb_hist_batch(context.handle, None, None, ctypes.byref(good), good_edges.ctypes.data,
                                          pattern.ctypes.data) == 1
        assert context.lib.mdb_hist_batch_dev(context.handle, ctypes.byref(dev.seg), None, ctypes.byref(good),
                                              good_edges.ctypes.data, None) == 1
        # the same request with good group ids works, in every form, and adds to what is there
        expected = pattern.reshape(3, 4) + _expected(batch, good_edges, inside[0], inside[1], groups, 3)
        request = Request(inside[0], inside[1], 3, 3, 0, 0)
        for form in ("host", "list", "dev"):
            counts = pattern.copy()
            assert _raw_hist(context, form, batch, dev, groups, dev_groups, request, good_edges, counts, dev_counts) == 0
            if form == "dev":
                counts = context.download_array(dev_counts, len(pattern), np.uint64)
            assert np.array_equal(counts.reshape(3, 4), expected), form
    finally:
        for pointer in (dev_groups, dev_bad_groups, dev_counts):
            context.dev_free(pointer)
        dev.free()


def test_malformed_segments_fail_as_the_range_aggregates_do(context):
    _, _, good = cases.mixed_batch(cases.LOSSLESS, False, seed=9, length=2000)
    rows = good.rows()
    streams = [k for k, row in enumerate(rows) if row[0] == mdb.MDB_MACAQUE_V_ID and len(row[6]) > 16]
    truncated = list(rows)
    k = streams[0]
    truncated[k] = truncated[k][:6] + (truncated[k][6][:len(truncated[k][6]) // 2],) + truncated[k][7:]
    unknown_type = list(rows)
    unknown_type[1] = (9,) + unknown_type[1][1:]
    edges = np.array([150.0], dtype=np.float32)
    for bad_rows in (truncated, unknown_type):
        batch = mdb.SegmentBatch.from_rows(bad_rows)
        with pytest.raises(mdb.HipError):
            context.agg_batch_range(batch, I64_MIN, I64_MAX, mdb.MDB_AGG_COUNT | mdb.MDB_AGG_SUM)
        counts = np.full((1, 2), PATTERN, dtype=np.uint64)
        for call in (lambda: context.hist(batch, edges, counts=counts), lambda: context.hist_list([batch], edges, counts=counts),
                     lambda: context.quantile(batch, [0.5])):
            with pytest.raises(mdb.HipError):
                call()
        dev = context.upload_segments(batch)
        try:
            with pytest.raises(mdb.HipError):
                context.hist_dev(dev, edges, counts=counts)
            with pytest.raises(mdb.HipError):
                context.quantile_dev(dev, [0.5])
        finally:
            dev.free()
        assert (counts == PATTERN).all()


def test_an_empty_batch_or_time_range_changes_nothing(context):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["abs5"], False, seed=8, length=2000)
    edges = np.array([120.0, 150.0], dtype=np.float32)
    groups = np.zeros(len(batch), dtype=np.uint32)
    empty = batch.slice(0, 0)
    last = int(batch.end_time.max())
    dev = context.upload_segments(batch)
    try:
        for t_lo, t_hi in ((last + 1, I64_MAX), (500, 400), (I64_MAX, I64_MIN)):
            counts = np.full((1, 3), PATTERN, dtype=np.uint64)
            context.hist(batch, edges, groups, t_lo, t_hi, counts=counts)
            context.hist_list([batch, empty], edges, None, t_lo, t_hi, counts=counts)
            context.hist_dev(dev, edges, groups, t_lo, t_hi, counts=counts)
            assert (counts == PATTERN).all()
        counts = np.full((2, 3), PATTERN, dtype=np.uint64)
        context.hist(empty, edges, counts=counts)
        context.hist_list([], edges, counts=counts)
        context.hist_list([empty, empty], edges, counts=counts)
        assert (counts == PATTERN).all()
    finally:
        dev.free()


# ---- quantiles ----------------------------------------------------------------------------------------------------

def _check_quantiles(context, batch, q, t_lo=None, t_hi=None, dev=None, what=None):
    timestamps, _, keys, _ = _grid(batch)
    lo_t, hi_t = _bounds(t_lo, t_hi)
    ordered = np.sort(keys[(timestamps >= lo_t) & (timestamps <= hi_t)])
    n = len(ordered)
    lo, hi, n_points = context.quantile(batch, q, t_lo, t_hi)
    assert n_points == n, what
    if n == 0:
        assert np.isnan(lo).all() and np.isnan(hi).all()  # (the wrapper's fill: untouched)
        return n
    positions = [(int(np.floor(np.float64(x) * np.float64(n - 1))), int(np.ceil(np.float64(x) * np.float64(n - 1)))) for x in q]
    expected_lo = _floats_of_keys(ordered[[p[0] for p in positions]])
    expected_hi = _floats_of_keys(ordered[[p[1] for p in positions]])
    assert np.array_equal(lo.view(np.uint32), expected_lo.view(np.uint32)), (what, q)
    assert np.array_equal(hi.view(np.uint32), expected_hi.view(np.uint32)), (what, q)
    if dev is not None:
        dev_lo, dev_hi, dev_n = context.quantile_dev(dev, q, t_lo, t_hi)
        assert dev_n == n and dev_lo.tobytes() == lo.tobytes() and dev_hi.tobytes() == hi.tobytes(), what
    return n


@pytest.mark.parametrize("eb_name,irregular", [("lossless", False), ("rel1", True), ("abs5", False)])
def test_quantiles_of_mixed_batches_are_the_sorted_grids(context, eb_name, irregular):
    _, _, batch = cases.mixed_batch(cases.error_bounds()[eb_name], irregular, seed=1300 + len(eb_name), length=20_000)
    timestamps = _grid(batch)[0]
    first, last = int(timestamps[0]), int(timestamps[-1])
    dev = context.upload_segments(batch)
    try:
        sizes = set()
        # the whole batch and the batch without its first point: an odd and an even N; under a time range; one point; none
        for t_lo, t_hi in ((None, None), (int(timestamps[1]), None), (first + (last - first) // 3, last - (last - first) // 4),
                           (int(timestamps[7]), int(timestamps[7])), (last + 1, None)):
            for q in (FIVE_Q, SIXTEEN_Q, [0.5]):
                sizes.add(_check_quantiles(context, batch, q, t_lo, t_hi, dev, (eb_name, t_lo, t_hi)))
        assert {n % 2 for n in sizes if n > 1} == {0, 1} and 1 in sizes and 0 in sizes
        # interpolation is the wrapper's: percentile_cont in f64
        timestamps, values, _, _ = _grid(batch)
        finite = np.sort(values.astype(np.float64))
        got, n_points = context.quantile(batch, [0.5, 0.999], interpolate=True)
        assert n_points == len(finite)
        assert np.allclose(got, np.quantile(finite, [0.5, 0.999]), rtol=1e-12, atol=0.0)
    finally:
        dev.free()


def test_quantiles_of_equal_and_repeated_values(context):
    def pmc(values, lengths):
        n = len(values)
        starts = np.concatenate([[0], np.cumsum(np.asarray(lengths[:-1], dtype=np.int64) * 10)])
        return scale_cases.simple_batch(np.full(n, scale_cases.PMC), starts, lengths, np.full(n, 10),
                                        np.asarray(values, dtype=np.float32), np.asarray(values, dtype=np.float32),
                                        np.zeros(n, dtype=bool))
    # every pass has all points in one cell
    equal = pmc([7.5, 7.5, 7.5], [100_000, 100_000, 100_000])
    lo, hi, n_points = context.quantile(equal, SIXTEEN_Q)
    assert n_points == 300_000 and (lo == 7.5).all() and (hi == 7.5).all()
    # values that repeat across the rank boundary (N even: ranks 49 999 and 50 000), and a boundary between two values
    for lengths, expected in (([60_000, 40_000], (1.0, 1.0)), ([50_000, 50_000], (1.0, 2.0)), ([49_999, 50_001], (2.0, 2.0))):
        batch = pmc([1.0, 2.0], lengths)
        lo, hi, n_points = context.quantile(batch, [0.5])
        assert (float(lo[0]), float(hi[0]), n_points) == expected + (100_000,)
        _check_quantiles(context, batch, FIVE_Q, what=lengths)
    one = pmc([3.25], [1])
    lo, hi, n_points = context.quantile(one, FIVE_Q)
    assert n_points == 1 and (lo == 3.25).all() and (hi == 3.25).all()


def test_quantiles_with_nan_and_signed_zeros(context):
    batch = cases.edge_case_batch()
    dev = context.upload_segments(batch)
    try:
        for q in (FIVE_Q, SIXTEEN_Q):
            _check_quantiles(context, batch, q, dev=dev, what="edge cases")
            _check_quantiles(context, batch, q, 150, 950, dev=dev, what="edge cases under a range")
    finally:
        dev.free()
    zeros = ora.try_compress_univariate_time_series(
        np.arange(6, dtype=np.int64) * 100, _f32([0x80000000, 0x00000000, 0x80000000, 0x00000000, 0x7FC00000, 0xFFC00000]),
        cases.LOSSLESS)
    lo, hi, n_points = context.quantile(zeros, [0.0, 0.3, 0.5, 1.0])
    assert n_points == 6
    assert lo.view(np.uint32).tolist() == [0xFFC00000, 0x80000000, 0x80000000, 0x7FC00000]
    assert hi.view(np.uint32).tolist() == [0xFFC00000, 0x80000000, 0x00000000, 0x7FC00000]


def test_quantile_errors_and_no_points_leave_the_outputs_untouched(context):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["abs5"], False, seed=5, length=3000)
    seg = batch.as_c()
    dev = context.upload_segments(batch)
    last = int(batch.end_time.max())
    try:
        for call, segments in ((context.lib.mdb_quantile_batch, seg), (context.lib.mdb_quantile_batch_dev, dev.seg)):
            def run(q, n_q, t_lo=I64_MIN, t_hi=I64_MAX, lo_null=False):
                lo, hi = np.full(17, 7.0, dtype=np.float32), np.full(17, 9.0, dtype=np.float32)
                n_points = ctypes.c_uint64(99)
                q = np.asarray(q, dtype=np.float64)
                code = call(context.handle, ctypes.byref(segments), t_lo, t_hi, q.ctypes.data, n_q,
                            None if lo_null else lo.ctypes.data, hi.ctypes.data, ctypes.byref(n_points))
                return code, n_points.value, bool((lo == 7.0).all() and (hi == 9.0).all())
            for q, n_q in (([0.5, 1.5], 2), ([np.nan], 1), ([-0.25], 1), ([0.5], 0), ([0.5] * 17, 17)):
                assert run(q, n_q) == (1, 99, True), (q, n_q)
            assert run([0.5], 1, lo_null=True)[0] == 1
            # no point inside the range: success, N = 0, the outputs as they were
            assert run(FIVE_Q, 5, last + 1, I64_MAX) == (0, 0, True)
            assert run(FIVE_Q, 5, 10, 5) == (0, 0, True)
            code, n_points, untouched = run([0.5], 1)
            assert code == 0 and n_points > 0 and not untouched
    finally:
        dev.free()
