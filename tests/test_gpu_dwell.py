"""The time spent per value cell per date_bin bucket on segments (mdb_dwell_buckets*): dwell[group][bucket][cell] in
microseconds. The tables are tests/comoments_cases.py's and hand-made batches of a handful of segments; the reference
(tests/dwell_cases.py) applies the linked rule to the oracle's grid row by row and walks every linked interval over the
buckets it crosses in Python integers.

Every comparison is assert_array_equal: the operator is integer arithmetic and there is no tolerance anywhere.
Expected values never come from the library under test, except in the tests that say they are consistency checks."""

import ctypes

import numpy as np
import pytest

import cases
import comoments_cases as cc
import datagen
import dwell_cases as dc
import hist_buckets_cases as hbc
import oracle_lib as ora
import modelardb_rs_amd as mdb

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
MAX_EDGES = mdb.MDB_HIST_MAX_EDGES
MAX_ROWS_UNDER_MAX_EDGES = 256   # (group, bucket) rows a request may have under the longest edge list: 8 MiB of counters


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()


def _span(field):
    return int(field.ts.min()), int(field.ts.max())


def _compress(timestamps, values, eb=cases.LOSSLESS):
    return ora.try_compress_univariate_time_series(np.asarray(timestamps, dtype=np.int64),
                                                   np.asarray(values, dtype=np.float32), eb)


def _edge_lists(values):
    """1 edge, about 16 edges through the data's range, MDB_HIST_MAX_EDGES edges through it."""
    lists = {"1": np.array([np.median(values)], dtype=np.float32), "16": dc.edges_through(values, 16),
             "max": dc.edges_through(values, MAX_EDGES)}
    assert len(lists["16"]) == 16 and len(lists["max"]) == MAX_EDGES
    return lists


def _check(hip, field, edges, groups, n_groups, origin, width, n_buckets, context, max_gap=None):
    got = hip.dwell_buckets(field.batch, edges, origin, width, n_buckets, groups=groups, max_gap=max_gap, n_groups=n_groups)
    expected = dc.oracle(field, edges, groups, n_groups, origin, width, n_buckets, max_gap)
    assert got.shape == (n_groups, n_buckets, len(edges) + 1) and got.dtype == np.uint64
    np.testing.assert_array_equal(got, expected, err_msg=context)
    return got


@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "one_group"])
@pytest.mark.parametrize("f", [0, 1, 2], ids=["lossless", "rel1", "abs5"])
def test_parity_with_the_rows_and_with_the_time_weighted_operator(hip, f, grouped):
    """All three model types, regular and irregular timestamps, segments far longer and far shorter than 64 rows;
    every bucket set of comoments_cases with its time range dropped, under 1, 16 and MDB_HIST_MAX_EDGES edges (the
    longest list where the request has at most 256 rows of cells, 4 groups x 64 buckets through the data among them);
    every cell compared. The cells of a row sum to
    integral_buckets' duration under STEP for the same request (a consistency check between two operators)."""
    field = cc.main_table()[f]
    groups, n_groups = (field.groups, 4) if grouped else (None, 1)
    lists = _edge_lists(field.values)
    filled = 0
    first, last = _span(field)
    # ... and 64 buckets cut through the data at an unaligned origin: with 4 groups the largest request the longest
    # edge list is run on, over every kind of segment at once
    through = ("64_buckets_unaligned", first - 777, (last - first + 777) // 64 + 13, 64, I64_MIN, I64_MAX)
    for name, origin, width, n_buckets, _, _ in cc.bucket_sets(first, last) + [through]:
        duration = hip.integral_buckets(field.batch, origin, width, n_buckets, groups=groups, method=mdb.MDB_INTEGRAL_STEP,
                                        n_groups=n_groups)["duration"]
        for edge_name, edges in lists.items():
            if edge_name == "max" and n_groups * n_buckets > MAX_ROWS_UNDER_MAX_EDGES:
                continue
            got = _check(hip, field, edges, groups, n_groups, origin, width, n_buckets, f"field {f} {name} {edge_name} edge(s)")
            np.testing.assert_array_equal(got.sum(axis=2, dtype=np.uint64), duration, err_msg=f"{name} {edge_name}")
            filled += int((got > 0).sum())
    assert filled > 10_000


def test_a_gapless_regular_series_is_delta_times_the_point_counts(hip):
    """Buckets aligned to the rows that end at or before the last row: every counted row holds its value for one whole
    sampling interval inside its bucket, so dwell == delta * hist_buckets (a consistency check), and both match their
    references."""
    for f in (0, 1, 2):
        field = cc.Field([cc.main_table()[f].parts[0]])
        first, last = _span(field)
        assert (np.diff(field.ts) == INTERVAL).all()
        edges = dc.edges_through(field.values, 16)
        for rows_per_bucket in (1, 7, 64):
            width = rows_per_bucket * INTERVAL
            n_buckets = (last - first) // width
            assert first + n_buckets * width <= last
            got = _check(hip, field, edges, None, 1, first, width, n_buckets, f"gapless {f} {rows_per_bucket}")
            counts = hip.hist_buckets(field.batch, edges, first, width, n_buckets)
            np.testing.assert_array_equal(counts, hbc.expected(field.batch, edges, (first, width, n_buckets, None, None)))
            np.testing.assert_array_equal(got, np.uint64(INTERVAL) * counts)


def test_finer_edges_finer_buckets_and_a_moved_origin(hip):
    """Merging adjacent cells of a finer edge list gives the cells of the coarser list it contains; buckets of width w
    summed in pairs equal buckets of width 2w; moving the origin by whole widths, with n_buckets moved along, gives
    the same numbers. Each side is also held to the reference."""
    for f in (0, 2):
        field = cc.main_table()[f]
        first, last = _span(field)
        fine = dc.edges_through(field.values, 16)
        coarse = fine[3::4]
        width = 1_700
        n_buckets = 2 * ((last - first + 40) // (2 * width) + 1)
        args = (field.groups, 4, first - 40, width, n_buckets)
        by_fine = _check(hip, field, fine, *args, "fine")
        by_coarse = _check(hip, field, coarse, *args, "coarse")
        np.testing.assert_array_equal(np.add.reduceat(by_fine, [0, 4, 8, 12, 16], axis=2), by_coarse)
        doubled = _check(hip, field, fine, field.groups, 4, first - 40, 2 * width, n_buckets // 2, "width 2w")
        np.testing.assert_array_equal(by_fine[:, 0::2] + by_fine[:, 1::2], doubled)
        for shift in (3, -2):   # (origin - shift * width: `shift` more buckets in front, or fewer)
            moved = _check(hip, field, fine, field.groups, 4, first - 40 - shift * width, width, n_buckets + shift, f"moved {shift}")
            if shift > 0:
                assert not moved[:, :shift].any()
                np.testing.assert_array_equal(moved[:, shift:], by_fine)
            else:
                np.testing.assert_array_equal(moved, by_fine[:, -shift:])


def test_links_across_buckets_by_hand(hip):
    """Two one-point segments: the only interval is the link between them, and the later value is never read."""
    field = cc.Field([_compress([130], [2.0]), _compress([370], [np.nan])])
    assert len(field.batch) == 2 and field.ts.tolist() == [130, 370]
    edges = np.array([1.0, 3.0], dtype=np.float32)
    # one link over three buckets, its first and last partial; buckets nothing reaches on either side
    got = _check(hip, field, edges, None, 1, 0, 100, 5, "three buckets")
    assert got[0, :, 1].tolist() == [0, 70, 100, 70, 0] and int(got.sum()) == 240
    # buckets that lie inside the link, and one that holds it whole
    got = _check(hip, field, edges, None, 1, 200, 10, 7, "inside")
    assert got[0, :, 1].tolist() == [10] * 7 and int(got.sum()) == 70
    got = _check(hip, field, edges, None, 1, -1_000, 10_000, 1, "whole")
    assert got[0, 0].tolist() == [0, 240, 0]
    # both points outside every bucket
    got = _check(hip, field, edges, None, 1, 140, 100, 2, "both ends outside")
    assert got[0, :, 1].tolist() == [100, 100]
    # a link over 100 buckets at an origin that cuts both ends
    far = cc.Field([_compress([0], [1.0]), _compress([10_000], [3.0])])
    got = _check(hip, far, edges, None, 1, 50, 100, 99, "hundred buckets")
    assert (got[0, :, 1] == 100).all() and int(got.sum()) == 9_900
    assert hip.dwell(far.batch, edges).tolist() == [[0, 10_000, 0]]


def _ramp(n, first_value, step, t0=1_000):
    """A Swing segment of n rows on regular timestamps: an exact line under an absolute bound."""
    timestamps = t0 + np.arange(n, dtype=np.int64) * INTERVAL
    values = (first_value + step * np.arange(n)).astype(np.float32)
    part = _compress(timestamps, values, cases.error_bounds()["abs5"])
    assert len(part) == 1 and part.model_type_id[0] == mdb.MDB_SWING_ID
    return part


def test_swing_segments(hip):
    """Ascending and descending lines that cross many cells inside one bucket (the binary searches of the closed form,
    and, under the longest edge list, its point-by-point path), with bucket edges on rows and between two rows."""
    up, down = _ramp(400, 100.0, 0.5), _ramp(400, 300.0, -0.5, t0=100_000)
    field = cc.Field([up, down])
    first, last = _span(field)
    assert (np.diff(field.values[:400]) > 0).all() and (np.diff(field.values[400:]) < 0).all()
    for edge_name, edges in _edge_lists(field.values).items():
        for origin, width in ((first - 10, last - first + 20), (first, 50 * INTERVAL), (first - 30, 250), (first + 1, 70),
                              (first - 7, 3_333)):
            n_buckets = (last - origin) // width + 2
            if edge_name == "max" and 2 * n_buckets > MAX_ROWS_UNDER_MAX_EDGES:
                continue
            got = _check(hip, field, edges, field.groups, 2, origin, width, n_buckets, f"swing {edge_name} {width}")
            assert got.sum(axis=(1, 2)).tolist() == [399 * INTERVAL - max(0, origin - first), 399 * INTERVAL]
            if width > 100 * INTERVAL:
                assert ((got > 0).sum(axis=2) > (8 if edge_name != "1" else 1)).any()   # (many cells inside one bucket)
    # one group: the descending line's first row lies behind the ascending line's last, so the two are linked
    edges = dc.edges_through(field.values, 16)
    got = _check(hip, field, edges, None, 1, first, 1_000, (last - first) // 1_000 + 1, "swing linked")
    assert int(got.sum()) == last - first


def test_segments_of_one_and_two_rows_and_short_runs(hip):
    """Series 3 of the main table (runs of 2..12 points) under every bound, and segments of 1..5 rows on irregular
    timestamps: as many links between segments as intervals inside them."""
    for f in (0, 1, 2):
        field = cc.Field([cc.main_table()[f].parts[3]])
        first, last = _span(field)
        edges = dc.edges_through(field.values, 16)
        for origin, width, n_buckets in ((first, last - first + 1, 1), (first, INTERVAL, (last - first) // INTERVAL + 1),
                                         (first - 33, 250, (last - first) // 250 + 2)):
            got = _check(hip, field, edges, None, 1, origin, width, n_buckets, f"short {f} {width}")
            assert int(got.sum()) == last - first
    rng = np.random.default_rng(5)
    n = 600
    timestamps = 1_000 + np.cumsum(rng.integers(1, 400, n))
    values = datagen.sine_series(9, n)[1]
    cuts = np.concatenate([[0], np.minimum(np.cumsum(rng.integers(1, 6, n)), n)])
    cuts = cuts[:int(np.argmax(cuts == n)) + 1]
    sizes = np.diff(cuts)
    assert (sizes == 1).sum() > 20 and (sizes == 2).sum() > 20
    tiny = cc.Field([_compress(timestamps[a:b], values[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(tiny.ts, timestamps) and len(tiny.batch) > n // 5
    first, last = _span(tiny)
    edges = dc.edges_through(values, 16)
    for origin, width, n_buckets in ((first - 55, 170, (last - first) // 170 + 2), (first, last - first, 1)):
        got = _check(hip, tiny, edges, None, 1, origin, width, n_buckets, f"tiny {width}")
        assert int(got.sum()) == last - first


def _is_regular(batch):
    return np.array([n == 0 or (batch.timestamps.value(i)[0] & 0x80) == 0 for i, n in enumerate(batch.timestamps.lengths())])


def test_a_pmc_mean_segment_that_is_all_residuals(hip):
    """The compressor writes no such segment, so one is cut by hand from a PMC-Mean segment on regular timestamps with
    a residual tail: the tail alone, its timestamps stream holding the tail's length, behind a one-row segment."""
    series = cc._series(600, False, (11, 12, 13), segment_length_range=(20, 120))
    source = cc.Field([_compress(series[0], series[1][2], cases.error_bounds()["abs5"])])
    batch, regular = source.batch, _is_regular(source.batch)
    tails = [i for i in range(len(batch)) if batch.model_type_id[i] == mdb.MDB_PMC_MEAN_ID and regular[i]
             and batch.residuals.lengths()[i] > 0 and 3 <= batch.residuals.value(i)[-1] < source.rows[i]]
    assert tails
    i = tails[0]
    n, r = int(source.rows[i]), int(batch.residuals.value(i)[-1])
    before = int(source.rows[:i].sum())
    timestamps, values = source.ts[before:before + n], source.values[before:before + n]
    row = batch.rows()[i]
    tail = mdb.SegmentBatch.from_rows([(row[0], int(timestamps[n - r]), int(timestamps[-1]), r.to_bytes(2, "big")) + row[4:]])
    lead = _compress([int(timestamps[n - r]) - INTERVAL], [values[0]])
    field = cc.Field([mdb.SegmentBatch.concat([lead, tail])])
    assert np.array_equal(field.ts[1:], timestamps[n - r:]) and field.values[1:].tobytes() == values[n - r:].tobytes()
    assert field.rows.tolist() == [1, r]
    first, last = _span(field)
    edges = dc.edges_through(field.values, 16) if len(np.unique(field.values)) > 1 else field.values[:1]
    for origin, width in ((first, INTERVAL), (first - 30, 70), (first + 1, 7), (first - 500, 1_300)):
        got = _check(hip, field, edges, None, 1, origin, width, (last - origin) // width + 2, f"all residuals {width}")
        assert int(got.sum()) == last - max(first, origin)
    # the source field, residual tails behind models of both kinds
    first, last = _span(source)
    _check(hip, source, dc.edges_through(source.values, 16), None, 1, first - 20, 370, (last - first) // 370 + 2, "tails")


def test_a_segment_without_rows_links_nothing_across_it(hip):
    """end_time < start_time under a stored length rebuilds to no row; the rows 200 and 500 are consecutive rows of the
    grid, so the expected counters are written out by hand."""
    left, right = _compress([100, 200], [1.0, 2.0]).rows(), _compress([500, 600], [2.0, 7.0]).rows()
    broken = mdb.SegmentBatch.from_rows(left + [(0, 400, 300, bytes([5]), 9.0, 9.0, b"", b"")] + right)
    timestamps, _, per_segment, _ = ora.grid_batch(broken)
    assert timestamps.tolist() == [100, 200, 500, 600] and per_segment.tolist()[len(left)] == 0
    edges = np.array([1.5], dtype=np.float32)
    got = hip.dwell_buckets(broken, edges, 0, 1_000, 1)
    assert got.tolist() == [[[100, 100]]]
    whole = cc.Field([mdb.SegmentBatch.from_rows(left + right)])   # without it the two are linked: 2.0 held on [200, 500)
    got = _check(hip, whole, edges, None, 1, 0, 1_000, 1, "no hole")
    assert got.tolist() == [[[100, 400]]]


def test_the_gap_rule(hip):
    """max_gap of 0, delta - 1 and delta inside a regular series, and of the seam's gap - 1, gap and gap + 1 across the
    hole between two segments of it."""
    source = cc.main_table()[0].parts[0]
    whole = cc.Field([source])
    hole_at = int(whole.rows[:len(source) // 2].sum())
    timestamps, values = whole.ts.copy(), whole.values
    timestamps[hole_at:] += 10 * INTERVAL + 3
    field = cc.Field([mdb.SegmentBatch.concat([_compress(timestamps[:hole_at], values[:hole_at]),
                                               _compress(timestamps[hole_at:], values[hole_at:])])])
    assert np.array_equal(field.ts, timestamps)
    seam = int(timestamps[hole_at] - timestamps[hole_at - 1])
    assert seam == 11 * INTERVAL + 3 and (np.delete(np.diff(timestamps), hole_at - 1) == INTERVAL).all()
    first, last = _span(field)
    edges = dc.edges_through(values, 16)
    args = (None, 1, first - 30, 7 * INTERVAL, (last - first) // (7 * INTERVAL) + 2)
    linked = {0: 0, INTERVAL - 1: 0, INTERVAL: last - first - seam, seam - 1: last - first - seam, seam: last - first,
              seam + 1: last - first, None: last - first}
    for max_gap, total in linked.items():
        got = _check(hip, field, edges, *args, f"max_gap {max_gap}", max_gap=max_gap)
        assert int(got.sum()) == total, max_gap
    # the three lossy and lossless fields of the irregular series under a gap some of its intervals exceed
    for f in (0, 1, 2):
        irregular = cc.Field([cc.main_table()[f].parts[1]])
        gaps = np.diff(irregular.ts)
        first, last = _span(irregular)
        for max_gap in (int(np.median(gaps)), int(gaps.max()) - 1):
            got = _check(hip, irregular, dc.edges_through(irregular.values, 16), None, 1, first - 9, 1_111,
                         (last - first) // 1_111 + 2, f"irregular {f} {max_gap}", max_gap=max_gap)
            assert int(got.sum()) == int(gaps[gaps <= max_gap].sum()) < last - first


def test_seams_without_a_link_and_groups(hip):
    edges = np.array([1.5, 4.5], dtype=np.float32)
    # time standing still: (500, 1) and (500, 2) are not linked; (500, 2) and (600, 4) are
    equal = cc.Field([_compress([500], [1.0]), _compress([500], [2.0]), _compress([600], [4.0])])
    assert equal.ts.tolist() == [500, 500, 600]
    assert _check(hip, equal, edges, None, 1, 0, 1_000, 1, "equal timestamps").tolist() == [[[0, 100, 0]]]
    # a step backwards across a seam links nothing; the rows inside the segments are linked
    backward = cc.Field([_compress([500, 600], [1.0, 2.0]), _compress([100, 250], [5.0, 7.0])])
    assert backward.ts.tolist() == [500, 600, 100, 250]
    assert _check(hip, backward, edges, None, 1, 0, 200, 4, "backward").tolist() == [[[0, 0, 100], [0, 0, 50], [100, 0, 0], [0, 0, 0]]]
    # a group change in mid-series: the link across the cut is gone, every other one stays
    series = cc.Field([cc.main_table()[1].parts[0]])
    first, last = _span(series)
    cut = len(series.batch) // 2
    groups = (np.arange(len(series.batch)) >= cut).astype(np.uint32)
    at = int(series.rows[:cut].sum())
    fine = dc.edges_through(series.values, 16)
    got = _check(hip, series, fine, groups, 2, first, 50 * INTERVAL, (last - first) // (50 * INTERVAL) + 1, "group change")
    assert got.sum(axis=(1, 2)).tolist() == [int(series.ts[at - 1]) - first, last - int(series.ts[at])]
    # a group per segment: only the links inside segments are left
    each = (np.arange(len(series.batch)) % 3).astype(np.uint32)
    got = _check(hip, series, fine, each, 3, first, 50 * INTERVAL, (last - first) // (50 * INTERVAL) + 1, "a group per segment")
    assert int(got.sum()) == int((series.batch.end_time - series.batch.start_time).sum())


def test_values_that_are_not_finite_and_both_zeros(hip):
    """NaN of both signs, both infinities and both zeros with an edge at +0.0: each is placed by its totalOrder key,
    and the durations stay exact."""
    bits = np.array([0xFFC00000, 0x80000000, 0x00000000, 0xFF800000, 0x7F800000, 0x7FC00000, 0xFFC00001, 0x3F800000],
                    dtype=np.uint32)
    values = bits.view(np.float32)
    timestamps = np.array([0, 10, 30, 60, 100, 150, 210, 280], dtype=np.int64)
    field = cc.Field([_compress(timestamps, values)])
    assert field.values.view(np.uint32).tolist() == bits.tolist()
    zero = np.array([0.0], dtype=np.float32)
    got = _check(hip, field, zero, None, 1, 0, 1_000, 1, "an edge at +0.0")
    assert got.tolist() == [[[10 + 20 + 40 + 70, 30 + 50 + 60]]]   # -NaN, -0.0, -inf, -NaN | +0.0, +inf, +NaN
    around = np.array([-np.inf, -0.0, 0.0, np.inf], dtype=np.float32)
    got = _check(hip, field, around, None, 1, 5, 100, 3, "edges at both infinities and both zeros")
    assert got[0].sum(axis=0).tolist() == [5 + 70, 40, 20, 30, 50 + 60]
    # the edge table of the other operators: NaN, +-0, +-inf and an epoch-scale Swing, each series a group
    for edge_field in cc.edge_table():
        first, last = _span(edge_field)
        n_groups = len(edge_field.parts)
        finite = edge_field.values[np.isfinite(edge_field.values)]
        edges = np.unique(np.concatenate([zero, dc.edges_through(finite, 16)]))
        for origin, width in ((first, 1 << 40), (first - 17, (last - first) // 50 + 1)):
            n_buckets = (last - origin) // width + 1
            got = _check(hip, edge_field, edges, edge_field.groups, n_groups, origin, width, n_buckets, f"edge table {width}")
            duration = hip.integral_buckets(edge_field.batch, origin, width, n_buckets, groups=edge_field.groups,
                                            method=mdb.MDB_INTEGRAL_STEP, n_groups=n_groups)["duration"]
            np.testing.assert_array_equal(got.sum(axis=2, dtype=np.uint64), duration)


def test_the_forms_and_two_runs_agree_and_a_call_adds(hip):
    field = cc.main_table()[1]
    batch, groups = field.batch, field.groups
    first, last = _span(field)
    edges = dc.edges_through(field.values, 16)
    args = (edges, first - 40, 2_900, (last - first + 40) // 2_900 + 1)
    expected = dc.oracle(field, edges, groups, 4, *args[1:])
    host = hip.dwell_buckets(batch, *args, groups=groups, n_groups=4)
    np.testing.assert_array_equal(host, expected)
    resident = field.resident(hip)
    dev = hip.dwell_buckets_dev(resident, *args, groups=groups, n_groups=4)
    again = hip.dwell_buckets_dev(resident, *args, groups=groups, n_groups=4)
    # the list cut inside series: links cross from one input to the next
    cuts = [0, 3, len(batch) // 3, len(batch) // 3 + 1, len(batch) - 2, len(batch)]
    listed = hip.dwell_buckets_list([batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])], *args,
                                    groups=[groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])], n_groups=4)
    assert host.tobytes() == dev.tobytes() == again.tobytes() == listed.tobytes()
    # ... while two calls over the same pieces lose the links across the cuts
    parts = [hip.dwell_buckets(batch.slice(a, b), *args, groups=groups[a:b], n_groups=4) for a, b in zip(cuts[:-1], cuts[1:])]
    assert int(sum(int(part.sum()) for part in parts)) < int(host.sum())
    # a call adds into counters that are not zero, in every form
    rng = np.random.default_rng(3)
    start = rng.integers(0, 1 << 40, host.shape).astype(np.uint64)
    for call in (lambda dwell: hip.dwell_buckets(batch, *args, groups=groups, dwell=dwell),
                 lambda dwell: hip.dwell_buckets_dev(resident, *args, groups=groups, dwell=dwell),
                 lambda dwell: hip.dwell_buckets_list([batch], *args, groups=[groups], dwell=dwell)):
        dwell = start.copy()
        assert call(dwell) is dwell
        np.testing.assert_array_equal(dwell, start + expected)
    assert mdb.dwell_merge(start.copy(), host).tobytes() == (start + expected).tobytes()
    # two calls over halves cut at a series boundary (no link crosses it) equal one call: with a group per series, and
    # with one group, where the series overlap in time and counters are added into
    cut = len(field.parts[0]) + len(field.parts[1])
    halves = (batch.slice(0, cut), batch.slice(cut, len(batch)))
    dwell = hip.dwell_buckets(halves[0], *args, groups=groups[:cut], n_groups=4)
    assert dwell[:2].any() and not dwell[2:].any()
    assert hip.dwell_buckets(halves[1], *args, groups=groups[cut:], dwell=dwell).tobytes() == host.tobytes()
    once = hip.dwell_buckets(batch, *args)
    np.testing.assert_array_equal(once, dc.oracle(field, edges, None, 1, *args[1:]))
    dwell = hip.dwell_buckets(halves[0], *args)
    second = hip.upload_segments(halves[1])
    assert hip.dwell_buckets_dev(second, *args, dwell=dwell).tobytes() == once.tobytes()
    second.free()
    # the shares of a row add up to one wherever the row holds time
    share = mdb.dwell_share(host)
    held = host.sum(axis=2) > 0
    assert np.isnan(share[~held]).all() and np.allclose(share[held].sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_the_convenience_is_one_bucket_over_the_span(hip):
    field = cc.main_table()[0]
    first, last = _span(field)
    edges = dc.edges_through(field.values, 16)
    got = hip.dwell(field.batch, edges, groups=field.groups, n_groups=4, max_gap=INTERVAL)
    assert got.shape == (4, 17)
    np.testing.assert_array_equal(got, dc.oracle(field, edges, field.groups, 4, first, last - first + 1, 1, INTERVAL)[:, 0])
    assert hip.dwell(field.batch.slice(0, 0), edges, n_groups=2).tolist() == [[0] * 17] * 2


def test_errors_leave_the_counters_untouched(hip):
    field = cc.main_table()[1]
    batch, groups = field.parts[0], np.arange(len(field.parts[0]), dtype=np.uint32) % 3
    rng = np.random.default_rng(9)
    edges = np.array([100.0, 150.0], dtype=np.float32)
    dwell = np.frombuffer(rng.bytes(3 * 10 * 3 * 8), dtype=np.uint64).reshape(3, 10, 3).copy()
    before = dwell.copy()
    resident = hip.upload_segments(batch)
    data = dwell.ctypes.data_as(ctypes.c_void_p)
    seg = batch.as_c()
    e = edges.ctypes.data_as(ctypes.c_void_p)

    def request(origin=0, width=1000, n_buckets=10, n_groups=3, max_gap=None, **fields):
        q = hip._dwell_request(origin, width, n_buckets, n_groups, max_gap)
        for name, value in fields.items():
            setattr(q.buckets if name in ("t_lo", "t_hi", "which_mask") else q, name, value)
        return q

    # the request's own errors, in the host form and - before `data` (a host pointer here) is touched - the device form
    for bad, message in ((request(width=0), b"width"), (request(width=-5), b"width"), (request(n_groups=0), b"n_groups"),
                         (request(which_mask=1), b"which_mask"), (request(t_lo=0), b"time range"),
                         (request(t_hi=10**9), b"time range"), (request(method=0), b"MDB_INTEGRAL_LINEAR"),
                         (request(method=7), b"Unknown method"), (request(flags=2), b"flags"), (request(max_gap=-1), b"max_gap"),
                         (request(n_buckets=1 << 58), b"overflows"), (request(n_buckets=1 << 44), b"do not fit")):
        for call in (lambda: hip.lib.mdb_dwell_buckets(hip.handle, ctypes.byref(seg), None, ctypes.byref(bad), e, 2, data),
                     lambda: hip.lib.mdb_dwell_buckets_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(bad), e, 2, data)):
            assert call() == 1
            assert message in hip.lib.mdb_last_error(), (message, hip.lib.mdb_last_error())
            assert dwell.tobytes() == before.tobytes()
    good = request()
    for wrong, n_edges, message in ((np.array([150.0, 100.0], dtype=np.float32), 2, b"strictly increasing"),
                                    (np.array([100.0, 100.0], dtype=np.float32), 2, b"strictly increasing"),
                                    (edges, 0, b"n_edges"), (edges, MAX_EDGES + 1, b"n_edges")):
        w = wrong.ctypes.data_as(ctypes.c_void_p)
        for call in (lambda: hip.lib.mdb_dwell_buckets(hip.handle, ctypes.byref(seg), None, ctypes.byref(good), w, n_edges, data),
                     lambda: hip.lib.mdb_dwell_buckets_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(good), w, n_edges, data)):
            assert call() == 1
            assert message in hip.lib.mdb_last_error(), (message, hip.lib.mdb_last_error())
            assert dwell.tobytes() == before.tobytes()
    for arguments in ((None, ctypes.byref(seg), None, ctypes.byref(good), e, 2, data), (hip.handle, None, None, ctypes.byref(good), e, 2, data),
                      (hip.handle, ctypes.byref(seg), None, None, e, 2, data), (hip.handle, ctypes.byref(seg), None, ctypes.byref(good), None, 2, data),
                      (hip.handle, ctypes.byref(seg), None, ctypes.byref(good), e, 2, None)):
        assert hip.lib.mdb_dwell_buckets(*arguments) == 1 and b"NULL" in hip.lib.mdb_last_error()
    assert dwell.tobytes() == before.tobytes()
    # a group id out of range, on a row no bucket reaches
    bad = groups.copy()
    bad[-1] = 3
    assert int(batch.start_time[-1]) > 10 * 1000 and int(batch.start_time[0]) < 10 * 1000
    for call in (lambda: hip.dwell_buckets(batch, edges, 0, 1000, 10, groups=bad, dwell=dwell, n_groups=3),
                 lambda: hip.dwell_buckets_list([batch.slice(0, 5), batch.slice(5, len(batch))], edges, 0, 1000, 10,
                                                groups=[bad[:5], bad[5:]], dwell=dwell, n_groups=3),
                 lambda: hip.dwell_buckets_dev(resident, edges, 0, 1000, 10, groups=bad, dwell=dwell, n_groups=3)):
        with pytest.raises(mdb.HipError, match="group id"):
            call()
        assert dwell.tobytes() == before.tobytes()
    resident.free()
    # a truncated values buffer on a reached segment: five points of MacaqueV values in five bytes
    pmc = lambda start, level: (0, start, start + 400, bytes([5]), level, level, b"", b"")
    truncated = mdb.SegmentBatch.from_rows([pmc(0, 1.5), (2, 500, 900, bytes([5]), 0.0, 0.0, bytes([1, 2, 3, 4, 0]), b""),
                                            pmc(1_000, 2.5)])
    one = np.frombuffer(rng.bytes(20 * 3 * 8), dtype=np.uint64).reshape(1, 20, 3).copy()
    one_before = one.copy()
    truncated_resident = hip.upload_segments(truncated)
    for call in (lambda: hip.dwell_buckets(truncated, edges, 0, 100, 20, dwell=one),
                 lambda: hip.dwell_buckets_dev(truncated_resident, edges, 0, 100, 20, dwell=one)):
        with pytest.raises(mdb.HipError, match="Malformed segment"):
            call()
        assert one.tobytes() == one_before.tobytes()
    truncated_resident.free()
    # the same segments without the broken one are fine: 1.5 is held up to the first row of the second segment
    whole = hip.dwell_buckets(mdb.SegmentBatch.from_rows([pmc(0, 1.5), pmc(1_000, 2.5)]), edges, 0, 100, 20)
    assert whole[0, :, 0].tolist() == [100] * 14 + [0] * 6 and not whole[0, :, 1:].any()


def test_nothing_to_do_succeeds_and_changes_nothing(hip):
    batch = cc.main_table()[1].parts[0]
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    rng = np.random.default_rng(10)
    edges = np.array([100.0, 150.0], dtype=np.float32)
    dwell = np.frombuffer(rng.bytes(3 * 10 * 3 * 8), dtype=np.uint64).reshape(3, 10, 3).copy()
    before = dwell.copy()
    resident = hip.upload_segments(batch)
    hip.dwell_buckets(batch.slice(0, 0), edges, 0, 100, 10, dwell=dwell, n_groups=3)
    hip.dwell_buckets_list([], edges, 0, 100, 10, dwell=dwell, n_groups=3)
    hip.dwell_buckets_list([batch.slice(0, 0), batch.slice(3, 3)], edges, 0, 100, 10, dwell=dwell, n_groups=3)
    # buckets no row reaches
    hip.dwell_buckets(batch, edges, int(batch.end_time.max()) + 1, 100, 10, groups=groups, dwell=dwell)
    hip.dwell_buckets_dev(resident, edges, -10_000, 100, 10, groups=groups, dwell=dwell)
    assert dwell.tobytes() == before.tobytes()
    none = np.zeros((3, 0, 3), dtype=np.uint64)
    assert hip.dwell_buckets(batch, edges, 0, 100, 0, groups=groups, dwell=none).shape == (3, 0, 3)
    assert hip.dwell_buckets_dev(resident, edges, 0, 100, 0, groups=groups, dwell=none).shape == (3, 0, 3)
    resident.free()
