"""Value histograms and exact quantiles per date_bin bucket and group (mdb_hist_buckets*, mdb_quantile_buckets*) against
the reference's plan GridExec -> AggregateExec GROUP BY the date_bin: the oracle's grid, every point put into its bucket
(floor((t - origin) / width), inside [0, n_buckets) and [t_lo, t_hi]) and group, then binned with numpy on totalOrder
keys (np.searchsorted(edge_keys, key, side="right")) or sorted by key per (group, bucket) - what tests/test_gpu_hist.py
does per group. Counts and order statistics are exact; the forms and two runs agree byte for byte.

Which edge lists meet which requests: every combination whose counters stay below MAX_COUNTERS (2^22 of them, 32 MB).
That leaves out only the 4 095-edge list under buckets of one interval (20 000 buckets x 4 096 cells x up to 5 groups:
3 GB a call); the 4 095 edges meet every other request, and the buckets of one interval every other edge list."""

import ctypes

import numpy as np
import pytest

import cases
import layouts
import oracle_lib as ora
import scale_cases
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
PATTERN = 0xA5A5A5A5A5A5A5A5
MAX_COUNTERS = 1 << 22
COUNT = mdb.MDB_AGG_COUNT
Q_LISTS = ([0.5], [0.0, 0.25, 0.5, 1.0], [0.999])

from hist_buckets_cases import (GRIDS as _GRIDS, keys_of as _keys, floats_of_keys as _floats_of_keys, f32 as _f32,
                                grid as _grid, placed as _placed, expected as _expected,
                                expected_quantiles as _expected_quantiles)


def _even_edges(keys, n_edges=4095):
    lo, hi = int(keys.min()), int(keys.max())
    picked = np.unique(np.linspace(lo, hi, n_edges + 2)[1:-1].astype(np.int64))
    picked = picked[(picked > lo) & (picked <= hi)] if hi > lo else np.array([lo], dtype=np.int64)
    return _floats_of_keys(picked)


def _edge_lists(batch):
    """One edge; seven edges ON rebuilt values and on their f32 neighbours; 4 095 edges even in key space between the
    grid's min and max; a list holding -0.0, +0.0, +inf and +NaN (those of tests/test_gpu_hist.py)."""
    keys = _grid(batch)[2]
    ordered = np.sort(keys)
    on_values = _floats_of_keys(ordered[[len(ordered) // 5, len(ordered) // 2, (4 * len(ordered)) // 5]])
    with np.errstate(over="ignore", invalid="ignore"):
        around = np.concatenate([np.nextafter(on_values, np.float32(-np.inf)), on_values,
                                 np.nextafter(on_values, np.float32(np.inf))])
    seven = _floats_of_keys(np.unique(_keys(around))[:7])
    return {"one": _floats_of_keys(ordered[[len(ordered) // 2]]), "seven": seven, "4095": _even_edges(keys),
            "specials": _f32([0x80000000, 0x00000000, 0x7F800000, 0x7FC00000])}


def _requests(batch):
    """{name: (origin, width, n_buckets, t_lo, t_hi)}: every way a bucket can cut a segment."""
    timestamps = _grid(batch)[0]
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    span = last - first + 1
    interval = int(np.median(np.diff(timestamps[:200]))) if len(timestamps) > 2 else 100
    interval = max(interval, 1)
    lengths = batch.end_time - batch.start_time
    model = batch.model_type_id != mdb.MDB_MACAQUE_V_ID
    longest = int(np.argmax(np.where(model, lengths, -1)))
    in_model = int(batch.start_time[longest] + lengths[longest] // 3)
    tails = np.flatnonzero(batch.residuals.lengths() > 0)
    in_tail = int(batch.end_time[tails[len(tails) // 2]]) - 1 if len(tails) else in_model + 1
    width = max(span // 37, 1)
    odd = max(33 * interval + 7, (span // 500) | 1)   # (at most 500 buckets where the data has gaps far wider than an interval)
    return {
        "a width that is no multiple of the interval": (first - 12_345, odd, (span + 12_345) // odd + 2, None, None),
        "an origin after the first point": (first + span // 5, width, 40, None, None),
        "buckets that stop before the last point": (first, width, 17, None, None),
        "t_lo and t_hi inside a bucket": (first - 50, width, 40, first + span // 7 + 3, last - span // 9 - 3),
        "t_lo inside a model part": (first, width, 40, in_model, None),
        "t_hi inside a residual tail": (first, width, 40, None, in_tail),
        "one bucket over everything": (first, span, 1, None, None),
        "buckets of one interval": (first, interval, min(span // interval + 1, 25_000), None, None),
        "a range without a point": (first, width, 40, last + 1, last + 1000),
    }


def _groupings(n):
    return [(None, 1), (np.arange(n, dtype=np.uint32) % 3, 3), (np.arange(n, dtype=np.uint32) % 3, 5)]


def _check_batch(hip, batch, what):
    half = len(batch) // 2
    halves = [batch.slice(0, half), batch.slice(half, len(batch))]
    dev = hip.upload_segments(batch)
    met = set()
    try:
        for edge_name, edges in _edge_lists(batch).items():
            for request_name, request in _requests(batch).items():
                origin, width, n_buckets, t_lo, t_hi = request
                for groups, n_groups in _groupings(len(batch)):
                    if n_groups * n_buckets * (len(edges) + 1) > MAX_COUNTERS:
                        continue
                    met.add((edge_name, request_name))
                    case = (what, edge_name, request_name, n_groups)
                    expected = _expected(batch, edges, request, groups, n_groups)
                    args = (edges, origin, width, n_buckets)
                    host = hip.hist_buckets(batch, *args, groups, t_lo, t_hi, n_groups=n_groups)
                    assert np.array_equal(host, expected), case
                    on_device = hip.hist_buckets_dev(dev, *args, groups, t_lo, t_hi, n_groups=n_groups)
                    listed = hip.hist_buckets_list(halves, *args, None if groups is None else [groups[:half], groups[half:]],
                                                   t_lo, t_hi, n_groups=n_groups)
                    again = hip.hist_buckets(batch, *args, groups, t_lo, t_hi, n_groups=n_groups)
                    assert host.tobytes() == on_device.tobytes() == listed.tobytes() == again.tobytes(), case
                    # a second call ADDS: the counts double, on the host and on the device
                    hip.hist_buckets(batch, *args, groups, t_lo, t_hi, counts=again)
                    hip.hist_buckets_dev(dev, *args, groups, t_lo, t_hi, counts=on_device)
                    assert np.array_equal(again, 2 * expected) and np.array_equal(on_device, 2 * expected), case
    finally:
        dev.free()
    requests, lists = set(_requests(batch)), set(_edge_lists(batch))
    assert {r for _, r in met} == requests and {e for e, _ in met} == lists
    assert {(e, r) for e in lists for r in requests} - met <= {("4095", "buckets of one interval")}


@pytest.mark.parametrize("irregular", [False, True], ids=["regular", "irregular"])
@pytest.mark.parametrize("eb_name", list(cases.error_bounds()))
def test_mixed_batches_match_the_binned_grid(hip, eb_name, irregular):
    _, _, batch = cases.mixed_batch(cases.error_bounds()[eb_name], irregular, seed=1400 + len(eb_name), length=20_000)
    assert len(_edge_lists(batch)["4095"]) == mdb.MDB_HIST_MAX_EDGES == 4095   # (the longest list the ABI takes)
    _check_batch(hip, batch, (eb_name, irregular))


@pytest.mark.parametrize("eb_name", ["lossless", "abs5"])
def test_edge_cases_nan_inf_and_zeros(hip, eb_name):
    _check_batch(hip, cases.edge_case_batch(cases.error_bounds()[eb_name]), eb_name)


# ---- the closed form of Swing, per bucket -------------------------------------------------------------------------

def _swing(length, first, last, decreasing=False, start=0, delta=1000):
    return scale_cases.simple_batch([scale_cases.SWING], [start], [length], [delta], [first], [last], [decreasing])


SWING_CASES = {
    "ascending": lambda: _swing(65_536, 100.0, 200.0),
    "descending": lambda: _swing(65_536, 100.0, 200.0, decreasing=True),
    "slope 0": lambda: _swing(65_536, 5.0, 5.0),
    "through zero": lambda: _swing(65_536, -5.0, 5.0),
    "both ends NaN, point by point": lambda: _swing(16, -np.inf, np.inf),
}


@pytest.mark.parametrize("name", list(SWING_CASES))
def test_swing_segments_in_closed_form_per_bucket(hip, name):
    """Single Swing segments on regular timestamps under 4 095 and 3 edges and 1, 7 and 1 000 buckets whose width is no
    multiple of the interval: the closed form is exact at every bucket boundary. The segment whose ends rebuild to NaN
    takes the point-by-point branch; the sign of its GENERATED NaNs is taken from grid_batch's rows, as
    tests/test_gpu_hist.py does and explains (IEEE 754 leaves it open; x86 and gfx950 differ)."""
    batch = SWING_CASES[name]()
    assert batch.model_type_id[0] == mdb.MDB_SWING_ID
    timestamps, values, keys, segment = _grid(batch)
    assert np.isnan(values).all() == ("NaN" in name)
    if "NaN" in name:
        row_timestamps, rows, _, _ = hip.grid_batch(batch)
        assert np.array_equal(row_timestamps, timestamps)
        assert np.array_equal(rows.view(np.uint32) & 0x7FFFFFFF, values.view(np.uint32) & 0x7FFFFFFF)
        values, keys = rows, _keys(rows)
        _GRIDS[id(batch)] = (batch, (timestamps, values, keys, segment))
    ordered = np.sort(keys)
    three = _floats_of_keys(np.unique(ordered[[len(ordered) // 4, len(ordered) // 2, (3 * len(ordered)) // 4]]))
    last = int(batch.end_time[0])
    for edges in (_even_edges(keys), three):
        for n_buckets in (1, 7, 1000):
            width = last // n_buckets + 1 + (3 if n_buckets > 1 else 0)
            for request in ((0, width, n_buckets, None, None), (-5, width, n_buckets, last // 3 + 1, last - last // 5)):
                expected = _expected(batch, edges, request)
                got = hip.hist_buckets(batch, edges, *request[:3], None, *request[3:])
                assert np.array_equal(got, expected), (name, len(edges), request)
                assert int(expected.sum()) > 0


# ---- metadata-only PMC-Mean: cells beyond 2^32 ----------------------------------------------------------------------

def _pmc_giants():
    if "giants" not in _GRIDS:
        n, points, delta = 5_000, 1_000_000, 10
        starts = np.arange(n, dtype=np.int64) * points * delta
        batch = scale_cases.simple_batch(np.full(n, scale_cases.PMC), starts, np.full(n, points), np.full(n, delta),
                                         np.full(n, 42.0, dtype=np.float32), np.full(n, 42.0, dtype=np.float32),
                                         np.zeros(n, dtype=bool))
        _GRIDS["giants"] = (batch, starts, points, delta)
    return _GRIDS["giants"]


def _giant_counts(starts, points, delta, groups, n_groups, origin, width, n_buckets, t_lo, t_hi):
    """Points per (group, bucket) of the giants by index arithmetic with Python integers."""
    out = np.zeros((n_groups, n_buckets), dtype=np.uint64)
    for i, start in enumerate(starts.tolist()):
        lo, hi = max(start, t_lo, origin), min(start + (points - 1) * delta, t_hi, origin + n_buckets * width - 1)
        if lo > hi:
            continue
        for b in range((lo - origin) // width, (hi - origin) // width + 1):
            a, z = max(lo, origin + b * width), min(hi, origin + (b + 1) * width - 1)
            k_lo, k_hi = -((start - a) // delta), (z - start) // delta
            if k_hi >= k_lo:
                out[groups[i], b] += k_hi - k_lo + 1
    return out


def test_cells_hold_more_than_32_bits(hip):
    """5 000 PMC-Mean segments of 10^6 regular points each (metadata only): one addition per (segment, bucket)."""
    batch, starts, points, delta = _pmc_giants()
    n = len(batch)
    edges = np.array([41.0, 43.0], dtype=np.float32)
    last = int(batch.end_time.max())
    counts = hip.hist_buckets(batch, edges, 0, last + 1, 1)
    assert counts.tolist() == [[[0, 5_000_000_000, 0]]]
    dev = hip.upload_segments(batch)
    try:
        assert hip.hist_buckets_dev(dev, edges, 0, last + 1, 1, counts=counts).tolist() == [[[0, 10_000_000_000, 0]]]
        # buckets of one and a half segments from an origin that is no multiple of the step, three groups, a range
        # that cuts the first and the last segment in the middle
        groups = np.arange(n, dtype=np.uint32) % 3
        origin, width = 5, 15_000_005
        n_buckets = (last - origin) // width + 1
        t_lo, t_hi = int(starts[0]) + 500_000 * delta, int(starts[-1]) + 499_999 * delta
        expected = _giant_counts(starts, points, delta, groups, 3, origin, width, n_buckets, t_lo, t_hi)
        assert int(expected.sum()) == 4_999_000_000 and int((expected > 0).sum()) > 3_000
        got = hip.hist_buckets_dev(dev, edges, origin, width, n_buckets, groups, t_lo, t_hi)
        assert np.array_equal(got[:, :, 1], expected) and not got[:, :, 0].any() and not got[:, :, 2].any()
        # the quantiles of a cell of more than 2^32 points, and of the cut cells
        lo, hi, n_points = hip.quantile_buckets_dev(dev, [0.5], 0, last + 1, 1)
        assert (lo.tolist(), hi.tolist(), n_points.tolist()) == ([[[42.0]]], [[[42.0]]], [[5_000_000_000]])
        lo, hi, n_points = hip.quantile_buckets_dev(dev, [0.0, 1.0], origin, width, n_buckets, groups, t_lo, t_hi)
        assert np.array_equal(n_points, expected)
        assert (lo[expected > 0] == 42.0).all() and (hi[expected > 0] == 42.0).all() and np.isnan(lo[expected == 0]).all()
    finally:
        dev.free()


# ---- malformed streams: timestamps that are not sorted ---------------------------------------------------------------

def _unsorted(batch, rng):
    """The batch with the timestamps of every second segment that has an irregular stream of six points or more out of
    order: interior neighbours swapped, the first and the last point kept (start_time and end_time stay the segment's
    bounds), the stream encoded again by the oracle. Returns the batch, the rows changed and their timestamps."""
    rows, changed, streams = list(batch.rows()), [], []
    for k, row in enumerate(rows):
        data = bytes(row[3])
        if len(data) == 0 or not data[0] & 0x80:
            continue
        timestamps = ora.decompress_all_timestamps(int(row[1]), int(row[2]), data)
        if len(timestamps) < 6 or (len(changed) + k) % 2:
            continue
        shuffled = timestamps.copy()
        for at in rng.choice(np.arange(1, len(timestamps) - 2), size=max(1, len(timestamps) // 4), replace=False):
            shuffled[at], shuffled[at + 1] = shuffled[at + 1], shuffled[at]
        if (np.diff(shuffled) >= 0).all():
            continue
        encoded = ora.compress_residual_timestamps(shuffled)
        assert np.array_equal(ora.decompress_all_timestamps(int(row[1]), int(row[2]), encoded), shuffled)
        rows[k] = row[:3] + (encoded,) + row[4:]
        changed.append(k)
        streams.append(shuffled)
    return mdb.SegmentBatch.from_rows(rows), changed, streams


@pytest.mark.parametrize("eb_name", ["lossless", "rel5", "abs5"])
def test_unsorted_timestamps_count_what_the_bucket_aggregates_count(hip, eb_name):
    """Segments whose irregular timestamps are not sorted (a malformed stream that still decodes) under MacaqueV values,
    residual tails and plain models, in buckets whose edges points out of order lie across: per (group,
    bucket) the cells add up to mdb_agg_buckets' COUNT and to mdb_moments_buckets' count - the points those operators
    take bucket by bucket - and n_points of the quantiles is the same number. A hand-made PMC-Mean segment without
    residuals is also checked point by point: each point lies in the bucket of its own timestamp."""
    _, _, sorted_batch = cases.mixed_batch(cases.error_bounds()[eb_name], True, seed=1700 + len(eb_name), length=3_000)
    batch, changed, streams = _unsorted(sorted_batch, np.random.default_rng(17))
    types = set(batch.model_type_id[changed].tolist())
    assert len(changed) >= 5 and (eb_name != "lossless" or mdb.MDB_MACAQUE_V_ID in types)
    if eb_name != "lossless":
        assert (batch.residuals.lengths()[changed] > 0).any() and (batch.residuals.lengths()[changed] == 0).any()
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    edges = np.array([120.0, 150.0, 180.0], dtype=np.float32)
    dev = hip.upload_segments(batch)
    try:
        # (a lane walks an unsorted stream once per bucket it reaches: about 64 and 23 buckets over the data keep that short)
        for origin, width, t_lo, t_hi in ((first, (last - first) // 64 | 1, None, None),
                                          (first - 77, (last - first) // 23, first + 5_555, last - 4_444)):
            n_buckets = (last - origin) // width + 1
            crossing = sum(int(((t[:-1] > t[1:]) & ((t[:-1] - origin) // width != (t[1:] - origin) // width)).sum()) for t in streams)
            assert crossing >= 3, "points out of order must lie across bucket edges"
            args = (origin, width, n_buckets)
            states = hip.agg_buckets(batch, *args, groups=groups, t_lo=t_lo, t_hi=t_hi, which_mask=COUNT, n_groups=3)
            moments = hip.moments_buckets(batch, *args, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
            assert np.array_equal(states["count"], moments["count"]) and int(states["count"].sum()) > 2_000
            counts = hip.hist_buckets(batch, edges, *args, groups, t_lo, t_hi, n_groups=3)
            assert np.array_equal(counts.sum(axis=2).astype(np.int64), states["count"]), (eb_name, width)
            assert hip.hist_buckets_dev(dev, edges, *args, groups, t_lo, t_hi, n_groups=3).tobytes() == counts.tobytes()
            _, _, n_points = hip.quantile_buckets_dev(dev, [0.5], *args, groups, t_lo, t_hi, 3)
            assert np.array_equal(n_points.astype(np.int64), states["count"]), (eb_name, width)
    finally:
        dev.free()


def test_an_unsorted_model_only_segment_places_every_point_by_its_own_timestamp(hip):
    timestamps = np.array([1000, 1100, 1300, 1200, 1400, 1650, 1500, 1600, 1900, 1800, 1700, 2000, 2100], dtype=np.int64)
    stream = ora.compress_residual_timestamps(timestamps)
    assert stream[0] & 0x80 and np.array_equal(ora.decompress_all_timestamps(1000, 2100, stream), timestamps)
    batch = mdb.SegmentBatch.from_rows([(mdb.MDB_PMC_MEAN_ID, 1000, 2100, stream, 7.5, 7.5, b"", b"")])
    edges = np.array([7.0, 8.0], dtype=np.float32)
    for origin, width, n_buckets, t_lo, t_hi in ((1000, 250, 5, None, None), (950, 100, 12, 1150, 1850), (1000, 1101, 1, None, None)):
        t_lo_, t_hi_ = I64_MIN if t_lo is None else t_lo, I64_MAX if t_hi is None else t_hi
        keep = (timestamps >= t_lo_) & (timestamps <= t_hi_) & (timestamps >= origin) & ((timestamps - origin) // width < n_buckets)
        expected = np.zeros((1, n_buckets, 3), dtype=np.uint64)
        expected[0, :, 1] = np.bincount((timestamps[keep] - origin) // width, minlength=n_buckets)
        got = hip.hist_buckets(batch, edges, origin, width, n_buckets, None, t_lo, t_hi)
        assert np.array_equal(got, expected), (origin, width)
        states = hip.agg_buckets(batch, origin, width, n_buckets, t_lo=t_lo, t_hi=t_hi, which_mask=COUNT)
        assert np.array_equal(states["count"], expected[:, :, 1].astype(np.int64))
        lo, hi, n_points = hip.quantile_buckets(batch, [0.0, 1.0], origin, width, n_buckets, None, t_lo, t_hi)
        assert np.array_equal(n_points, expected[:, :, 1]) and (lo[n_points > 0] == 7.5).all() and (hi[n_points > 0] == 7.5).all()


# ---- invariants -----------------------------------------------------------------------------------------------------

def test_invariants_against_the_other_operators(hip):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["rel1"], True, seed=77, length=20_000)
    edges = _edge_lists(batch)["seven"]
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    for t_lo, t_hi in ((first, last), (first + 12_345, last - 23_456)):
        width = (t_hi - t_lo) // 23 + 1
        args = (t_lo, width, 23)
        counts = hip.hist_buckets(batch, edges, *args, groups, t_lo, t_hi, n_groups=3)
        # summed over buckets that cover the range: Context.hist of the range
        assert np.array_equal(counts.sum(axis=1), hip.hist(batch, edges, groups, t_lo, t_hi, n_groups=3))
        # summed over cells: agg_buckets' COUNT
        states = hip.agg_buckets(batch, *args, groups=groups, t_lo=t_lo, t_hi=t_hi, which_mask=COUNT, n_groups=3)
        assert np.array_equal(counts.sum(axis=2).astype(np.int64), states["count"])
        assert int(counts.sum()) > 10_000
        # one bucket: the bytes of hist
        one = hip.hist_buckets(batch, edges, t_lo, t_hi - t_lo + 1, 1, groups, t_lo, t_hi, n_groups=3)
        assert one.tobytes() == hip.hist(batch, edges, groups, t_lo, t_hi, n_groups=3).tobytes()


# ---- quantiles ------------------------------------------------------------------------------------------------------

def _check_quantiles(hip, batch, dev, request, q, groups, n_groups, what):
    origin, width, n_buckets, t_lo, t_hi = request
    e_lo, e_hi, e_n, filled = _expected_quantiles(batch, request, q, groups, n_groups)
    lo, hi, n_points = hip.quantile_buckets(batch, q, origin, width, n_buckets, groups, t_lo, t_hi, n_groups)
    assert np.array_equal(n_points, e_n), what
    assert np.array_equal(lo.view(np.uint32)[filled], e_lo[filled]), what
    assert np.array_equal(hi.view(np.uint32)[filled], e_hi[filled]), what
    assert np.isnan(lo[~filled]).all() and np.isnan(hi[~filled]).all(), what   # (the wrapper's fill: untouched)
    d_lo, d_hi, d_n = hip.quantile_buckets_dev(dev, q, origin, width, n_buckets, groups, t_lo, t_hi, n_groups)
    assert (d_lo.tobytes(), d_hi.tobytes(), d_n.tobytes()) == (lo.tobytes(), hi.tobytes(), n_points.tobytes()), what
    states = hip.agg_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, which_mask=COUNT,
                             n_groups=n_groups)
    assert np.array_equal(n_points.astype(np.int64), states["count"]), what
    return set(np.unique(n_points).tolist())


@pytest.mark.parametrize("eb_name,irregular", [("lossless", False), ("rel1", True), ("abs5", False), ("lossless", True)])
def test_quantiles_of_mixed_batches_are_the_sorted_cells(hip, eb_name, irregular):
    _, _, batch = cases.mixed_batch(cases.error_bounds()[eb_name], irregular, seed=1500 + len(eb_name), length=20_000)
    requests = _requests(batch)
    dev = hip.upload_segments(batch)
    try:
        sizes = set()
        for request_name in ("a width that is no multiple of the interval", "t_lo and t_hi inside a bucket",
                             "t_hi inside a residual tail", "buckets of one interval", "a range without a point",
                             "one bucket over everything"):
            for groups, n_groups in _groupings(len(batch))[:2] if "one interval" in request_name else _groupings(len(batch)):
                for q in Q_LISTS:
                    sizes |= _check_quantiles(hip, batch, dev, requests[request_name], q, groups, n_groups,
                                              (eb_name, irregular, request_name, n_groups, q))
        assert 0 in sizes and 1 in sizes and {n % 2 for n in sizes if n > 1} == {0, 1}
        # one bucket and one group: Context.quantile, bit for bit
        first, last = int(batch.start_time.min()), int(batch.end_time.max())
        for t_lo, t_hi in ((first, last), (first + 54_321, last - 12_345)):
            for q in Q_LISTS:
                lo, hi, n_points = hip.quantile_buckets(batch, q, t_lo, t_hi - t_lo + 1, 1, None, t_lo, t_hi)
                whole = hip.quantile(batch, q, t_lo, t_hi)
                assert (lo.tobytes(), hi.tobytes(), int(n_points[0, 0])) == (whole[0].tobytes(), whole[1].tobytes(), whole[2])
        # q = 0 and q = 1: the v_min / v_max of m4_buckets, bit for bit
        groups = np.arange(len(batch), dtype=np.uint32) % 3
        origin, width, n_buckets, t_lo, t_hi = requests["t_lo and t_hi inside a bucket"]
        lo, hi, n_points = hip.quantile_buckets(batch, [0.0, 1.0], origin, width, n_buckets, groups, t_lo, t_hi, 3)
        cells = hip.m4_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
        filled = n_points > 0
        assert filled.sum() > 50 and np.array_equal(n_points.astype(np.int64), cells["count"])
        for out in (lo, hi):
            assert np.array_equal(out[..., 0].view(np.uint32)[filled], cells["v_min"].view(np.uint32)[filled])
            assert np.array_equal(out[..., 1].view(np.uint32)[filled], cells["v_max"].view(np.uint32)[filled])
        # interpolation is the wrapper's: percentile_cont in f64, per cell
        values, n_again = hip.quantile_buckets(batch, [0.5, 0.95], origin, width, n_buckets, groups, t_lo, t_hi, 3,
                                               interpolate=True)
        rows, keys = _placed(batch, requests["t_lo and t_hi inside a bucket"], groups)
        assert np.array_equal(n_again, n_points)
        for row in np.flatnonzero(filled.reshape(-1))[:40]:
            cell = np.sort(_floats_of_keys(keys[rows == row]).astype(np.float64))
            assert np.allclose(values.reshape(-1, 2)[row], np.quantile(cell, [0.5, 0.95]), rtol=1e-12, atol=0.0)
        assert np.isnan(values[~filled]).all()
    finally:
        dev.free()


def test_quantiles_of_equal_and_repeated_values(hip):
    def pmc(values, lengths):
        n = len(values)
        starts = np.concatenate([[0], np.cumsum(np.asarray(lengths[:-1], dtype=np.int64) * 10)])
        return scale_cases.simple_batch(np.full(n, scale_cases.PMC), starts, lengths, np.full(n, 10),
                                        np.asarray(values, dtype=np.float32), np.asarray(values, dtype=np.float32),
                                        np.zeros(n, dtype=bool))
    # every pass has all points of a cell in one digit
    equal = pmc([7.5, 7.5, 7.5], [100_000, 100_000, 100_000])
    lo, hi, n_points = hip.quantile_buckets(equal, [0.0, 0.3, 0.5, 1.0], 0, 1_000_000, 3)
    assert n_points.tolist() == [[100_000] * 3] and (lo == 7.5).all() and (hi == 7.5).all()
    # two buckets of 100 000 points each, the values repeating across the rank boundary (ranks 49 999 and 50 000) of
    # the first and meeting at the boundary in the second
    batch = pmc([1.0, 2.0, 1.0, 2.0], [60_000, 40_000, 50_000, 50_000])
    lo, hi, n_points = hip.quantile_buckets(batch, [0.5], 0, 1_000_000, 2)
    assert n_points.tolist() == [[100_000, 100_000]]
    assert (lo[0, :, 0].tolist(), hi[0, :, 0].tolist()) == ([1.0, 1.0], [1.0, 2.0])
    batch = pmc([1.0, 2.0], [49_999, 50_001])
    lo, hi, n_points = hip.quantile_buckets(batch, [0.5], 0, 1_000_000, 1)
    assert (float(lo[0, 0, 0]), float(hi[0, 0, 0]), int(n_points[0, 0])) == (2.0, 2.0, 100_000)
    one = pmc([3.25], [1])
    lo, hi, n_points = hip.quantile_buckets(one, [0.0, 0.5, 1.0], 0, 10, 2)
    assert n_points.tolist() == [[1, 0]] and (lo[0, 0] == 3.25).all() and (hi[0, 0] == 3.25).all()
    assert np.isnan(lo[0, 1]).all() and np.isnan(hi[0, 1]).all()


def test_quantiles_with_nan_and_signed_zeros(hip):
    batch = cases.edge_case_batch()
    dev = hip.upload_segments(batch)
    try:
        # (the series lie at 0 .. 40 000, near 1.66e12 and at 2^41: three requests of a few buckets, not one over all)
        assert int(batch.start_time.min()) == 0 and int(batch.end_time.max()) > 1 << 40
        late = int(batch.start_time[batch.start_time > 1 << 40].min()) if (batch.start_time > 1 << 40).any() else 1 << 40
        for request in ((0, 8_000, 5, None, None), (-3, 170, 8, 150, 950), (late - 100, 100_000, 8, None, None)):
            for q in Q_LISTS:
                _check_quantiles(hip, batch, dev, request, q, None, 1, ("edge cases", request, q))
    finally:
        dev.free()
    zeros = ora.try_compress_univariate_time_series(
        np.arange(12, dtype=np.int64) * 100,
        _f32([0x80000000, 0x00000000, 0x80000000, 0x00000000, 0x7FC00000, 0xFFC00000] * 2), cases.LOSSLESS)
    lo, hi, n_points = hip.quantile_buckets(zeros, [0.0, 0.3, 0.5, 1.0], 0, 600, 2)
    assert n_points.tolist() == [[6, 6]]
    for bucket in range(2):
        assert lo[0, bucket].view(np.uint32).tolist() == [0xFFC00000, 0x80000000, 0x80000000, 0x7FC00000]
        assert hi[0, bucket].view(np.uint32).tolist() == [0xFFC00000, 0x80000000, 0x00000000, 0x7FC00000]


def test_the_passes_do_not_depend_on_the_number_of_cells(hip):
    """The launches of the counting kernel for one mdb_quantile_buckets_dev call are MDB_QUANTILE_BUCKETS_PASSES, with one
    cell and with 3 x 1 000 cells, for one rank and for eight."""
    _, _, batch = cases.mixed_batch(cases.error_bounds()["rel1"], False, seed=31, length=20_000)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    dev = hip.upload_segments(batch)
    hip.profile_enable(True)
    try:
        seen = []
        for q in ([0.5], [0.1, 0.5, 0.95, 0.99]):
            for n_buckets, use_groups in ((1, None), (1000, groups)):
                hip.profile_reset()
                _, _, n_points = hip.quantile_buckets_dev(dev, q, first, (last - first) // n_buckets + 1, n_buckets, use_groups)
                profile = hip.profile()
                assert int(n_points.sum()) == 20_000
                seen.append((profile["k_hist_buckets_window"][0], profile["k_quantile_select"][0]))
        assert seen == [(mdb.MDB_QUANTILE_BUCKETS_PASSES, mdb.MDB_QUANTILE_BUCKETS_PASSES)] * 4
        assert mdb.MDB_QUANTILE_BUCKETS_PASSES <= 4
    finally:
        hip.profile_enable(False)
        dev.free()


# ---- errors ---------------------------------------------------------------------------------------------------------

def _raw(hip, operator, form, batch, dev, groups, dev_groups, request, extra, n_extra, outputs, dev_counts):
    """One raw call - the return code. operator "hist": extra = edges, outputs = [counts] (dev: dev_counts);
    "quantile": extra = q, outputs = [lo, hi, n_points] (host pointers in both forms)."""
    lib, seg = hip.lib, batch.as_c()
    extra_pointer = None if extra is None else extra.ctypes.data_as(ctypes.c_void_p)
    request_pointer = None if request is None else ctypes.byref(request)
    host_groups = None if groups is None else groups.ctypes.data
    device_groups = None if dev_groups is None else ctypes.c_void_p(dev_groups)
    if operator == "quantile":
        out = [a.ctypes.data for a in outputs]
        if form == "host":
            return lib.mdb_quantile_buckets(hip.handle, ctypes.byref(seg), host_groups, request_pointer, extra_pointer,
                                            n_extra, *out)
        return lib.mdb_quantile_buckets_dev(hip.handle, ctypes.byref(dev.seg), device_groups, request_pointer,
                                            extra_pointer, n_extra, *out)
    if form == "host":
        return lib.mdb_hist_buckets(hip.handle, ctypes.byref(seg), host_groups, request_pointer, extra_pointer, n_extra,
                                    outputs[0].ctypes.data)
    if form == "list":
        pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
        group_pointers = (ctypes.c_void_p * 1)(host_groups)
        return lib.mdb_hist_buckets_list(hip.handle, pointers, group_pointers, 1, request_pointer, extra_pointer, n_extra,
                                         outputs[0].ctypes.data)
    return lib.mdb_hist_buckets_dev(hip.handle, ctypes.byref(dev.seg), device_groups, request_pointer, extra_pointer,
                                    n_extra, ctypes.c_void_p(dev_counts))


def test_errors_leave_the_outputs_untouched(hip):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["abs5"], False, seed=5, length=3000)
    n = len(batch)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    good_edges = np.array([120.0, 150.0, 180.0], dtype=np.float32)
    good_q = np.array([0.5, 0.9], dtype=np.float64)
    Request = _abi.BucketRequestC
    groups = np.arange(n, dtype=np.uint32) % 3
    bad_groups = groups.copy()
    bad_groups[n - 1] = 3  # (the last segment: outside the time range of the request below)
    inside = (first, int(batch.start_time[n - 1]) - 1)
    width = (last - first) // 2 + 1
    good = Request(first, width, 2, I64_MIN, I64_MAX, 3, 0)
    pattern = np.full(3 * 2 * 4, PATTERN, dtype=np.uint64)
    dev = hip.upload_segments(batch)
    dev_groups, dev_bad_groups = hip.upload_array(groups), hip.upload_array(bad_groups)
    dev_counts = hip.upload_array(pattern)
    # name: (request, groups / device groups, what the operator-specific argument is replaced by)
    common = {
        "which_mask": (Request(first, width, 2, I64_MIN, I64_MAX, 3, COUNT), groups, dev_groups),
        "width 0": (Request(first, 0, 2, I64_MIN, I64_MAX, 3, 0), groups, dev_groups),
        "a negative width": (Request(first, -width, 2, I64_MIN, I64_MAX, 3, 0), groups, dev_groups),
        "no groups": (Request(first, width, 2, I64_MIN, I64_MAX, 0, 0), None, None),
        "cells that overflow": (Request(first, 1, 1 << 62, I64_MIN, I64_MAX, 0xFFFFFFFF, 0), None, None),
        # (2^32 - 1 groups of 2^13 buckets: 2^45 rows, more counters than any device holds)
        "cells that fit no device": (Request(first, 1, 1 << 13, I64_MIN, I64_MAX, 0xFFFFFFFF, 0), None, None),
        "a group id out of range, outside the time range": (Request(first, width, 2, inside[0], inside[1], 3, 0),
                                                            bad_groups, dev_bad_groups),
        "NULL request": (None, groups, dev_groups),
    }
    bad_edges = {
        "no edges": (good_edges, 0), "4096 edges": (np.arange(4096, dtype=np.float32), 4096),
        "equal edges": (np.array([1, 1, 2], dtype=np.float32), 3), "descending edges": (np.array([3, 2, 1], dtype=np.float32), 3),
        "-0.0 after +0.0": (_f32([0x00000000, 0x80000000, 0x3F800000]), 3), "NULL edges": (None, 3),
    }
    bad_q = {"q above 1": (np.array([0.5, 1.5]), 2), "q below 0": (np.array([-0.25]), 1), "q NaN": (np.array([np.nan]), 1),
             "no q": (good_q, 0), "five q": (np.full(5, 0.5), 5), "NULL q": (None, 1)}

    def fresh_outputs():
        return [np.full(3 * 2 * 5, 7.0, dtype=np.float32), np.full(3 * 2 * 5, 9.0, dtype=np.float32), np.full(6, 99, dtype=np.uint64)]

    def check_hist(name, request, host_groups, device_groups, edges, n_edges):
        for form in ("host", "list", "dev"):
            counts = pattern.copy()
            code = _raw(hip, "hist", form, batch, dev, host_groups, device_groups, request, edges, n_edges, [counts], dev_counts)
            assert code == 1 and hip.lib.mdb_last_error(), (name, form)
            assert np.array_equal(counts, pattern), (name, form)
            assert np.array_equal(hip.download_array(dev_counts, len(pattern), np.uint64), pattern), (name, form)

    def check_quantile(name, request, host_groups, device_groups, q, n_q):
        for form in ("host", "dev"):
            outputs = fresh_outputs()
            code = _raw(hip, "quantile", form, batch, dev, host_groups, device_groups, request, q, n_q, outputs, None)
            assert code == 1 and hip.lib.mdb_last_error(), (name, form)
            assert (outputs[0] == 7.0).all() and (outputs[1] == 9.0).all() and (outputs[2] == 99).all(), (name, form)

    try:
        for name, (request, host_groups, device_groups) in common.items():
            check_hist(name, request, host_groups, device_groups, good_edges, 3)
            check_quantile(name, request, host_groups, device_groups, good_q, 2)
        for name, (edges, n_edges) in bad_edges.items():
            check_hist(name, good, groups, dev_groups, edges, n_edges)
        for name, (q, n_q) in bad_q.items():
            check_quantile(name, good, groups, dev_groups, q, n_q)
        # NULL batches and outputs
        assert hip.lib.mdb_hist_buckets(hip.handle, None, None, ctypes.byref(good), good_edges.ctypes.data, 3, pattern.ctypes.data) == 1
        assert hip.lib.mdb_hist_buckets_dev(hip.handle, ctypes.byref(dev.seg), None, ctypes.byref(good), good_edges.ctypes.data, 3, None) == 1
        outputs = fresh_outputs()
        assert hip.lib.mdb_quantile_buckets_dev(hip.handle, ctypes.byref(dev.seg), None, ctypes.byref(good), good_q.ctypes.data, 2,
                                                None, outputs[1].ctypes.data, outputs[2].ctypes.data) == 1
        assert hip.lib.mdb_quantile_buckets(hip.handle, ctypes.byref(batch.as_c()), None, ctypes.byref(good), good_q.ctypes.data, 2,
                                            outputs[0].ctypes.data, outputs[1].ctypes.data, None) == 1
        # the same request with good group ids works, in every form, and adds to what is there
        request = Request(first, width, 2, inside[0], inside[1], 3, 0)
        as_tuple = (first, width, 2, inside[0], inside[1])
        expected = pattern.reshape(3, 2, 4) + _expected(batch, good_edges, as_tuple, groups, 3)
        for form in ("host", "list", "dev"):
            counts = pattern.copy()
            assert _raw(hip, "hist", form, batch, dev, groups, dev_groups, request, good_edges, 3, [counts], dev_counts) == 0
            if form == "dev":
                counts = hip.download_array(dev_counts, len(pattern), np.uint64)
            assert np.array_equal(counts.reshape(3, 2, 4), expected), form
        # (a third bucket behind the data: cells with N == 0 beside the filled ones)
        request, as_tuple = Request(first, width, 3, inside[0], inside[1], 3, 0), (first, width, 3, inside[0], inside[1])
        e_lo, e_hi, e_n, filled = _expected_quantiles(batch, as_tuple, good_q, groups, 3)
        for form in ("host", "dev"):
            outputs = [np.full(40, 7.0, dtype=np.float32), np.full(40, 9.0, dtype=np.float32), np.full(9, 99, dtype=np.uint64)]
            assert _raw(hip, "quantile", form, batch, dev, groups, dev_groups, request, good_q, 2, outputs, None) == 0
            assert np.array_equal(outputs[2].reshape(3, 3), e_n) and filled.any() and not filled.all()
            lo, hi = outputs[0][:18].reshape(3, 3, 2), outputs[1][:18].reshape(3, 3, 2)
            assert np.array_equal(lo.view(np.uint32)[filled], e_lo[filled]) and np.array_equal(hi.view(np.uint32)[filled], e_hi[filled])
            assert (lo[~filled] == 7.0).all() and (hi[~filled] == 9.0).all()   # (N == 0: untouched)
            assert (outputs[0][18:] == 7.0).all() and (outputs[1][18:] == 9.0).all()
    finally:
        for pointer in (dev_groups, dev_bad_groups, dev_counts):
            hip.dev_free(pointer)
        dev.free()


def test_malformed_segments_fail_as_the_range_aggregates_do(hip):
    _, _, good = cases.mixed_batch(cases.LOSSLESS, False, seed=9, length=2000)
    rows = good.rows()
    streams = [k for k, row in enumerate(rows) if row[0] == mdb.MDB_MACAQUE_V_ID and len(row[6]) > 16]
    truncated = list(rows)
    k = streams[0]
    truncated[k] = truncated[k][:6] + (truncated[k][6][:len(truncated[k][6]) // 2],) + truncated[k][7:]
    unknown_type = list(rows)
    unknown_type[1] = (9,) + unknown_type[1][1:]
    edges = np.array([150.0], dtype=np.float32)
    first, last = int(good.start_time.min()), int(good.end_time.max())
    args = (first, (last - first) // 4 + 1, 4)
    for bad_rows in (truncated, unknown_type):
        batch = mdb.SegmentBatch.from_rows(bad_rows)
        with pytest.raises(mdb.HipError):
            hip.agg_batch_range(batch, I64_MIN, I64_MAX, mdb.MDB_AGG_COUNT | mdb.MDB_AGG_SUM)
        counts = np.full((1, 4, 2), PATTERN, dtype=np.uint64)
        dev = hip.upload_segments(batch)
        try:
            for call in (lambda: hip.hist_buckets(batch, edges, *args, counts=counts),
                         lambda: hip.hist_buckets_list([batch], edges, *args, counts=counts),
                         lambda: hip.hist_buckets_dev(dev, edges, *args, counts=counts),
                         lambda: hip.quantile_buckets(batch, [0.5], *args),
                         lambda: hip.quantile_buckets_dev(dev, [0.5], *args)):
                with pytest.raises(mdb.HipError, match="Malformed"):
                    call()
        finally:
            dev.free()
        assert (counts == PATTERN).all()


def test_empty_inputs_change_nothing(hip):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["abs5"], False, seed=8, length=2000)
    edges = np.array([120.0, 150.0], dtype=np.float32)
    groups = np.zeros(len(batch), dtype=np.uint32)
    empty = batch.slice(0, 0)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    dev = hip.upload_segments(batch)
    try:
        for t_lo, t_hi in ((last + 1, I64_MAX), (500, 400), (I64_MAX, I64_MIN)):
            counts = np.full((1, 4, 3), PATTERN, dtype=np.uint64)
            hip.hist_buckets(batch, edges, first, 100_000, 4, groups, t_lo, t_hi, counts=counts)
            hip.hist_buckets_list([batch, empty], edges, first, 100_000, 4, None, t_lo, t_hi, counts=counts)
            hip.hist_buckets_dev(dev, edges, first, 100_000, 4, groups, t_lo, t_hi, counts=counts)
            assert (counts == PATTERN).all()
            for lo, hi, n_points in (hip.quantile_buckets(batch, [0.5], first, 100_000, 4, groups, t_lo, t_hi),
                                     hip.quantile_buckets_dev(dev, [0.5], first, 100_000, 4, groups, t_lo, t_hi)):
                assert not n_points.any() and np.isnan(lo).all() and np.isnan(hi).all()
        # buckets that lie after the data, an empty batch, no bucket at all
        counts = np.full((2, 4, 3), PATTERN, dtype=np.uint64)
        hip.hist_buckets(batch, edges, last + 1, 1000, 4, counts=counts)
        hip.hist_buckets(empty, edges, first, 1000, 4, counts=counts)
        hip.hist_buckets_list([], edges, first, 1000, 4, counts=counts)
        hip.hist_buckets_list([empty, empty], edges, first, 1000, 4, counts=counts)
        assert (counts == PATTERN).all()
        assert hip.hist_buckets(batch, edges, first, 1000, 0).shape == (1, 0, 3)
        assert hip.hist_buckets_dev(dev, edges, first, 1000, 0).shape == (1, 0, 3)
        lo, hi, n_points = hip.quantile_buckets(empty, [0.5], first, 1000, 4)
        assert not n_points.any() and np.isnan(lo).all() and np.isnan(hi).all()
        assert hip.quantile_buckets(batch, [0.5], first, 1000, 0)[2].shape == (1, 0)
    finally:
        dev.free()


# ---- layouts and resident batches ---------------------------------------------------------------------------------------

def _layout_requests(batch):
    """Two requests of 37 intervals a bucket over the layouts corpus, in front of and behind its gap of 2^40 (those of
    tests/test_gpu_moments.py)."""
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    behind = batch.start_time > first + (1 << 41)
    assert 20 < int(behind.sum()) < len(batch) - 20
    front_last = int(batch.end_time[batch.end_time < first + (1 << 40)].max())
    behind_first = int(batch.start_time[behind].min())
    width = 3700
    requests = [(first - 33, width, (front_last - first) // width + 2), (behind_first - 33, width, (last - behind_first) // width + 2)]
    assert all(n_buckets < 5_000 for _, _, n_buckets in requests), requests
    return requests


_PLAIN = {}


def _layout_results(hip, batch):
    edges = np.array([-1.0, 0.0, 50.0, 100.0, 150.0, 1000.0], dtype=np.float32)
    out = []
    for args in _layout_requests(batch):
        out.append(hip.hist_buckets(batch, edges, *args).tobytes())
        out.extend(a.tobytes() for a in hip.quantile_buckets(batch, [0.0, 0.5, 0.99], *args))
    return out


@pytest.mark.parametrize("mode", layouts.MODES)
def test_layouts_give_the_bytes_of_the_plain_layout(hip, mode):
    batch = layouts.corpus(20_000)[0]
    if "plain" not in _PLAIN:
        _PLAIN["plain"] = _layout_results(hip, batch)
        edges = np.array([-1.0, 0.0, 50.0, 100.0, 150.0, 1000.0], dtype=np.float32)
        for k, args in enumerate(_layout_requests(batch)):
            expected = _expected(batch, edges, args + (None, None))
            assert np.frombuffer(_PLAIN["plain"][4 * k], dtype=np.uint64).tolist() == expected.reshape(-1).tolist()
            assert int((expected.sum(axis=2) > 0).sum()) > 100
    assert _layout_results(hip, layouts.relayout(batch, mode, 7)) == _PLAIN["plain"]


def test_resident_batches_give_the_same_bytes_in_any_order_and_context(hip):
    _, _, batch = cases.mixed_batch(cases.LOSSLESS, True, seed=41, length=20_000)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    edges = _edge_lists(batch)["seven"]
    args = (edges, first - 7, (last - first) // 61 + 1, 62, groups)
    resident = hip.upload_segments(batch)
    clone = hip.clone()
    try:
        before = hip.hist_buckets_dev(resident, *args)
        assert np.array_equal(before, _expected(batch, edges, args[1:4] + (None, None), groups, 3))
        quantiles = hip.quantile_buckets_dev(resident, [0.5, 0.99], *args[1:])
        hip.agg_buckets_dev(resident, *args[1:4], groups=groups)
        hip.quantile_dev(resident, [0.5])
        hip.grid_resident(resident)
        assert hip.hist_buckets_dev(resident, *args).tobytes() == before.tobytes()
        again = hip.quantile_buckets_dev(resident, [0.5, 0.99], *args[1:])
        assert [a.tobytes() for a in again] == [a.tobytes() for a in quantiles]
        assert clone.hist_buckets_dev(resident, *args).tobytes() == before.tobytes()
        assert [a.tobytes() for a in clone.quantile_buckets_dev(resident, [0.5, 0.99], *args[1:])] == [a.tobytes() for a in quantiles]
    finally:
        clone.close()
        resident.free()
