"""The value of a series at regular instants on segments (mdb_sample_at*): per instant and group the number of
contributions and their f64 sum, LINEAR (interpolate), STEP (last observation carried forward) and EXACT (rows only).
The reference (tests/sample_cases.py) applies the linked rule to the oracle's grid row by row and rules (a) and (b) of
the contract in exact rational arithmetic.

Tolerances are the contract's: count equal in every cell; |sum - exact| <= 2^-48 * sum max(|v0|, |v1|) over the cell's
contributions; a cell with count == 1 on a series' own grid holds the grid's float bit for bit; a cell with a
non-finite value that its method reads has a non-finite sum and an exact count. Expected values never come from the
library under test, except in the tests that say they are consistency checks. The shapes are small: a few thousand
rows in tens to a few hundred segments."""

import ctypes

import numpy as np
import pytest

import cases
import comoments_cases as cc
import datagen
import oracle_lib as ora
import sample_cases as sc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
CELL = mdb.SAMPLE_CELL_DTYPE
LINEAR, STEP, EXACT = mdb.MDB_SAMPLE_LINEAR, mdb.MDB_SAMPLE_STEP, mdb.MDB_SAMPLE_EXACT
METHODS = sc.METHODS
EDGE_EPOCH = 1658671178037  # the first timestamp of the edge cases' epoch-scale series

_TABLE = {}


def small_table():
    """Three fields (lossless, 1 % relative, absolute 5) of four short series: regular and irregular timestamps,
    segments of 20..120 rows, a sine, runs of 2..12 points. Series 0 and the sine overlap in time."""
    if "fields" not in _TABLE:
        sine_ts = 5_000 + np.arange(800, dtype=np.int64) * INTERVAL
        sines = [datagen.sine_series(k, 800)[1] for k in (3, 4, 5)]
        series = [cc._series(600, False, (11, 12, 13), segment_length_range=(20, 120)),
                  cc._series(500, True, (21, 22, 23), segment_length_range=(20, 120), t0=3_000),
                  (sine_ts, sines), cc._series(200, False, (31, 32, 33), segment_length_range=(2, 12), t0=70_000)]
        bounds = cases.error_bounds()
        _TABLE["fields"] = cc.table(series, [bounds["lossless"], bounds["rel1"], bounds["abs5"]])
    return _TABLE["fields"]


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()
    for field in _TABLE.get("fields", []):
        field.free()


def _span(field):
    return int(field.ts.min()), int(field.ts.max())


def _compress(timestamps, values, eb=cases.LOSSLESS):
    return ora.try_compress_univariate_time_series(np.asarray(timestamps, dtype=np.int64),
                                                   np.asarray(values, dtype=np.float32), eb)


def _is_regular(batch):
    return np.array([n == 0 or (batch.timestamps.value(i)[0] & 0x80) == 0
                     for i, n in enumerate(batch.timestamps.lengths())])


def _check(hip, field, groups, n_groups, origin, width, n, context, methods=METHODS, max_gap=None):
    """sample_at against the reference under each method: {method: (cells, expected)}."""
    out = {}
    for method, name in methods:
        got = hip.sample_at(field.batch, origin, width, n, groups=groups, method=method, max_gap=max_gap,
                            n_groups=n_groups)
        expected = sc.oracle(field, groups, n_groups, origin, width, n, method, max_gap)
        sc.assert_cells(got, expected, f"{context} {name}")
        out[method] = (got, expected)
    return out


def test_the_table_holds_every_kind_of_segment():
    """The precondition of the parity test below, from the segments alone."""
    seen = set()
    for field in small_table():
        batch = field.batch
        regular, tail = _is_regular(batch), batch.residuals.lengths() > 0
        for i in range(len(batch)):
            seen.add((int(batch.model_type_id[i]), bool(regular[i]), bool(tail[i])))
    for model in (mdb.MDB_PMC_MEAN_ID, mdb.MDB_SWING_ID):
        for is_regular in (True, False):
            for has_tail in (True, False):
                assert (model, is_regular, has_tail) in seen, (model, is_regular, has_tail)
    assert (mdb.MDB_MACAQUE_V_ID, True, False) in seen and (mdb.MDB_MACAQUE_V_ID, False, False) in seen


@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "one_group"])
@pytest.mark.parametrize("f", [0, 1, 2], ids=["lossless", "rel1", "abs5"])
def test_parity_with_the_rows_in_exact_arithmetic(hip, f, grouped):
    """All three model types on regular and irregular timestamps, with and without a residual tail; a width below the
    sampling interval (several instants inside one interval), the interval itself, widths above a segment's length
    (segments without a pair), instants before and behind all data. One group: series 0 and the sine overlap, so
    cells hold two contributions."""
    field = small_table()[f]
    assert np.isfinite(field.values).all()
    groups, n_groups = (field.groups, 4) if grouped else (None, 1)
    first, last = _span(field)
    span = last - first + 1
    most = 0
    for name, origin, width, n in (("width_7", first + 4_000, 7, 1_500),
                                   ("width_70", first - 30, 70, span // 70 + 3),
                                   ("own_interval", first, INTERVAL, span // INTERVAL + 1),
                                   ("unaligned_3333", first - 12_345, 3_333, (span + 12_345) // 3_333 + 2),
                                   ("width_20000", first - 1, 20_000, span // 20_000 + 2),
                                   ("one_instant", first + 40_000, span, 1),
                                   ("before_the_data", first - 5_000, INTERVAL, 40),
                                   ("behind_the_data", last + 1, 1_000, 50)):
        results = _check(hip, field, groups, n_groups, origin, width, n, f"field {f} {name} {n_groups} group(s)")
        most = max(most, int(results[LINEAR][1]["count"].max()))
        if name in ("before_the_data", "behind_the_data"):
            assert all(int(cells["count"].sum()) == 0 for cells, _ in results.values())
        np.testing.assert_array_equal(results[LINEAR][0]["count"], results[STEP][0]["count"])
        assert (results[EXACT][0]["count"] <= results[LINEAR][0]["count"]).all()
    assert most == 1 if grouped else most >= 2


def test_a_series_on_its_own_grid_is_the_grid_bit_for_bit(hip):
    """The exact promise: width == the sampling interval at the series' first timestamp. Every cell has count 1 and
    the float of mdb_grid_batch, under all three methods - NaN payloads and the sign of zero included."""
    fields = [cc.Field([small_table()[f].parts[k]]) for f in (0, 1, 2) for k in (0, 2)]
    fields += [cc.Field([cc.edge_table()[f].parts[k]]) for f in (0, 1)
               for k, (name, _, _) in enumerate(cases.edge_case_series())
               if name in ("specials", "nan_run", "inf_run", "residuals_255", "leading_residuals", "swing_then_residuals",
                           "tiny_values")]
    for number, field in enumerate(fields):
        first, last = _span(field)
        assert (np.diff(field.ts) == INTERVAL).all()
        for method, name in METHODS:
            got = hip.sample_at(field.batch, first, INTERVAL, len(field.ts), method=method)
            assert (got["count"] == 1).all(), (number, name)
            assert got["sum"][0].astype(np.float32).tobytes() == field.values.tobytes(), (number, name)
            assert got["sum"][0].tobytes() == field.values.astype(np.float64).tobytes(), (number, name)
            with np.errstate(invalid="ignore"):
                assert mdb.sample_values(got)[0].astype(np.float32).tobytes() == field.values.tobytes(), (number, name)


def test_seams_links_and_short_segments(hip):
    """Segments of one and two rows; instants on a segment's first row, on its last row, on the neighbour's first row
    and strictly inside the link between two segments."""
    # two one-row segments, (0, 1.0) and (10 000, 3.0): the only interval is the link between them
    field = cc.Field([_compress([0], [1.0]), _compress([10_000], [3.0])])
    assert len(field.batch) == 2 and field.ts.tolist() == [0, 10_000] and field.values.tolist() == [1.0, 3.0]
    for origin, n in ((0, 101), (50, 100), (-300, 110)):
        results = _check(hip, field, None, 1, origin, 100, n, f"link {origin}")
        at = origin + 100 * np.arange(n)
        inside = (at > 0) & (at < 10_000)
        rows = (at == 0) | (at == 10_000)
        for method, level in ((LINEAR, 1.0 + 2.0 * at / 10_000), (STEP, np.ones(n))):
            got = results[method][0][0]
            np.testing.assert_array_equal(got["count"], (inside | rows).astype(np.uint64))
            assert np.allclose(got["sum"][inside], level[inside], rtol=1e-15, atol=0.0)
        np.testing.assert_array_equal(results[EXACT][0][0]["count"], rows.astype(np.uint64))
        if origin == 0:
            assert results[LINEAR][0]["sum"][0, [0, 25, 100]].tolist() == [1.0, 1.5, 3.0]
    # a one-row, a two-row and a longer segment of one series, cut by hand: the seams lie on instants
    timestamps = np.arange(40, dtype=np.int64) * INTERVAL + 700
    values = datagen.sine_series(2, 40)[1]
    cuts = [0, 1, 3, 4, 6, 25, 26, 40]
    for eb in (cases.LOSSLESS, cases.error_bounds()["abs5"]):
        pieces = cc.Field([mdb.SegmentBatch.concat([_compress(timestamps[a:b], values[a:b], eb)
                                                    for a, b in zip(cuts[:-1], cuts[1:])])])
        assert np.array_equal(pieces.ts, timestamps) and (pieces.rows[:4] <= 2).all()
        for origin, width, n in ((700, INTERVAL, 40), (700, 50, 79), (690, 20, 200), (650, 300, 15)):
            _check(hip, pieces, None, 1, origin, width, n, f"pieces {origin} {width}")
    # segments of 1..5 rows on irregular timestamps: as many links between segments as intervals inside them
    rng = np.random.default_rng(5)
    n = 400
    timestamps = 1_000 + np.cumsum(rng.integers(1, 400, n))
    values = datagen.sine_series(9, n)[1]
    cuts = np.concatenate([[0], np.minimum(np.cumsum(rng.integers(1, 6, n)), n)])
    cuts = cuts[:int(np.argmax(cuts == n)) + 1]
    tiny = cc.Field([mdb.SegmentBatch.concat([_compress(timestamps[a:b], values[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])])
    assert np.array_equal(tiny.ts, timestamps) and len(tiny.batch) > n // 5
    first, last = _span(tiny)
    for origin, width in ((first - 55, 170), (first, 13), (first, 5_000)):
        results = _check(hip, tiny, None, 1, origin, width, (last - origin) // width + 2, f"tiny {width}")
        # every instant inside [first, last] is defined once under LINEAR and STEP: nothing is lost at a seam
        at = origin + width * np.arange((last - origin) // width + 2)
        np.testing.assert_array_equal(results[STEP][0]["count"][0], ((at >= first) & (at <= last)).astype(np.uint64))


def test_equal_timestamps_and_a_group_change(hip):
    # equal timestamps at a seam: (500, 1) and (500, 2) are not linked and both lie on the instant; (500, 2) and
    # (600, 4) are linked
    equal = cc.Field([mdb.SegmentBatch.concat([_compress([400, 500], [0.5, 1.0]), _compress([500], [2.0]),
                                               _compress([600], [4.0])])])
    assert equal.ts.tolist() == [400, 500, 500, 600]
    results = _check(hip, equal, None, 1, 400, 50, 6, "equal timestamps")
    linear, step, exact = (results[m][0][0] for m in (LINEAR, STEP, EXACT))
    assert linear["count"].tolist() == [1, 1, 2, 1, 1, 0] and linear["sum"].tolist() == [0.5, 0.75, 3.0, 3.0, 4.0, 0.0]
    assert step["count"].tolist() == [1, 1, 2, 1, 1, 0] and step["sum"].tolist() == [0.5, 0.5, 3.0, 2.0, 4.0, 0.0]
    assert exact["count"].tolist() == [1, 0, 2, 0, 1, 0] and exact["sum"].tolist() == [0.5, 0.0, 3.0, 0.0, 4.0, 0.0]
    # a group change in the middle of a series: the link between the two segments is lost, nothing else
    series = cc.Field([small_table()[1].parts[0]])
    first, last = _span(series)
    cut = len(series.batch) // 2
    groups = (np.arange(len(series.batch)) >= cut).astype(np.uint32)
    rows_before = int(series.rows[:cut].sum())
    t0, t1 = int(series.ts[rows_before - 1]), int(series.ts[rows_before])
    assert t1 - t0 == INTERVAL
    n = (last - first) // 20 + 1
    results = _check(hip, series, groups, 2, first, 20, n, "group change")
    at = first + 20 * np.arange(n)
    lost = (at > t0) & (at < t1)
    assert lost.sum() == 4
    for method in (LINEAR, STEP):
        count = results[method][0]["count"]
        np.testing.assert_array_equal(count.sum(axis=0), (~lost).astype(np.uint64))
        assert count[0, at > t0].sum() == 0 and count[1, at < t1].sum() == 0


def test_the_gap_rule(hip):
    field = cc.Field([small_table()[0].parts[0], small_table()[2].parts[0]])   # regular: MacaqueV, and PMC-Mean / Swing
    for k in (0, 1):
        series = cc.Field([field.parts[k]])
        first, last = _span(series)
        assert (np.diff(series.ts) == INTERVAL).all()
        args = (first - 30, 70, (last - first) // 70 + 2)
        # below the sampling interval only on-row instants are defined: EXACT and the others agree, bytes and all
        exact = hip.sample_at(series.batch, *args, method=EXACT)
        assert exact["count"].sum() > 0
        for max_gap in (INTERVAL - 1, 0):
            results = _check(hip, series, None, 1, *args, f"gap {max_gap} series {k}", max_gap=max_gap)
            for method in (LINEAR, STEP, EXACT):
                assert results[method][0].tobytes() == exact.tobytes()
        results = _check(hip, series, None, 1, *args, f"gap equal series {k}", max_gap=INTERVAL)
        for method, _ in METHODS:
            assert results[method][0].tobytes() == hip.sample_at(series.batch, *args, method=method).tobytes()
            assert results[method][0].tobytes() == hip.sample_at(series.batch, *args, method=method,
                                                                 max_gap=I64_MAX).tobytes()
        assert int(results[STEP][0]["count"].sum()) == (last - args[0]) // 70 - (first - args[0] - 1) // 70
    # holes of 10 and of 300 intervals inside an irregular segment, max_gap between them: exactly the long hole is lost
    n = 900
    steps = np.full(n - 1, INTERVAL, dtype=np.int64)
    steps[200], steps[600] = 10 * INTERVAL, 300 * INTERVAL
    timestamps = np.concatenate([[12_300], 12_300 + np.cumsum(steps)])
    for eb in (cases.LOSSLESS, cases.error_bounds()["abs5"]):
        holes = cc.Field([_compress(timestamps, datagen.sine_series(8, n)[1], eb)])
        assert np.array_equal(holes.ts, timestamps) and not _is_regular(holes.batch).all()
        first, last = _span(holes)
        for max_gap, lost in ((100 * INTERVAL, 300 * INTERVAL), (None, 0), (5 * INTERVAL, 310 * INTERVAL)):
            results = _check(hip, holes, None, 1, first, 50, (last - first) // 50 + 1, f"holes {max_gap}", max_gap=max_gap)
            # the instants strictly inside a hole longer than max_gap are the gaps; every other one is defined once
            at = first + 50 * np.arange((last - first) // 50 + 1)
            defined = np.ones(len(at), dtype=bool)
            for t0, t1 in zip(timestamps[:-1], timestamps[1:]):
                if max_gap is not None and t1 - t0 > max_gap:
                    defined &= ~((at > t0) & (at < t1))
            assert int((~defined).sum()) == lost // 50 - (0 if lost == 0 else 1 if lost == 300 * INTERVAL else 2)
            np.testing.assert_array_equal(results[LINEAR][0]["count"][0], defined.astype(np.uint64))
    # a gap between two segments, cut and kept
    pair = cc.Field([mdb.SegmentBatch.concat([_compress([0, 100, 200], [1.0, 2.0, 4.0]),
                                              _compress([10_000, 10_100], [3.0, 5.0])])])
    for max_gap, linked in ((9_799, False), (9_800, True)):
        results = _check(hip, pair, None, 1, 0, 50, 210, f"seam gap {max_gap}", max_gap=max_gap)
        count = results[LINEAR][0]["count"][0]
        assert count[:5].tolist() == [1] * 5 and count[200:203].tolist() == [1] * 3
        assert (count[5:200] == (1 if linked else 0)).all()


def test_many_series_in_one_group_take_the_sort_path(hip):
    """300 one-segment series in one group under 5 instants: runs of 300 equal keys out of order - the stable sort and
    two levels of the tree - and as many contributions per cell."""
    parts = [_compress(np.arange(6) * INTERVAL + (k % 7), np.full(6, 0.25 * k - 30.0)) for k in range(300)]
    field = cc.Field([mdb.SegmentBatch.concat(parts)])
    assert len(field.batch) == 300
    results = _check(hip, field, None, 1, 3, 110, 5, "300 series")
    assert int(results[LINEAR][1]["count"].max()) >= 250 and int(results[EXACT][1]["count"].max()) >= 40
    groups = (np.arange(300) % 3).astype(np.uint32)
    _check(hip, field, groups, 3, 3, 110, 5, "300 series, 3 groups")


@pytest.mark.parametrize("f", [0, 1], ids=["lossless", "abs5"])
def test_edge_table(hip, f):
    """NaN, +-0, +-inf, one- and two-point segments, residual tails of random bits, epoch-scale Swing, width 2^40:
    each series a group. count is exact everywhere; the sum is non-finite exactly where the reference says so."""
    field = cc.edge_table()[f]
    n_groups = len(field.parts)
    plain = special = 0
    for origin, width, n in ((0, 100, 40), (0, 50, 80), (-35, 25, 240), (EDGE_EPOCH - 1000, 500, 30 * 6),
                             (EDGE_EPOCH, 50_000, 10), (0, 1 << 40, 3), (5, 1, 400)):
        for method, name in METHODS:
            got = hip.sample_at(field.batch, origin, width, n, groups=field.groups, method=method, n_groups=n_groups)
            counts = sc.assert_cells(got, sc.oracle(field, field.groups, n_groups, origin, width, n, method),
                                     f"edge {origin} {width} {name}")
            plain, special = plain + counts[0], special + counts[1]
    assert plain > 0 and special > 0   # (both kinds of cell were among them)


def test_a_pmc_mean_segment_that_is_all_residuals(hip):
    """The compressor writes no such segment, so one is cut by hand from a PMC-Mean segment on regular timestamps with
    a residual tail: the tail alone, its timestamps stream holding the tail's length. The tail is seeded with the last
    rebuilt value before it, so a one-row segment of the model's value stands in front."""
    source = small_table()[2]
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
    assert field.rows.tolist() == [1, r] and int(tail.residuals.value(0)[-1]) == r   # (every row of it is a residual)
    first, last = _span(field)
    for origin, width in ((first, INTERVAL), (first - 30, 70), (first + 1, 7), (first - 500, 1_300)):
        _check(hip, field, None, 1, origin, width, (last - origin) // width + 2, f"all residuals {width}")
    for method, name in METHODS:
        got = hip.sample_at(field.batch, first, INTERVAL, r + 1, method=method)
        assert (got["count"] == 1).all() and got["sum"][0].astype(np.float32).tobytes() == field.values.tobytes(), name


def test_timestamps_and_origins_near_both_int64_ends(hip):
    rng = np.random.default_rng(3)
    values = datagen.sine_series(7, 300)[1]
    low, high = I64_MIN + 3, I64_MAX - 299 * INTERVAL
    offsets = np.concatenate([[0], np.cumsum(rng.integers(1, 200, 299))]).astype(np.int64)
    for eb in (cases.LOSSLESS, cases.error_bounds()["rel1"]):
        for base, timestamps in ((low, low + np.arange(300, dtype=np.int64) * INTERVAL),
                                 (high, high + np.arange(300, dtype=np.int64) * INTERVAL),
                                 (low, low + offsets), (I64_MAX - int(offsets[-1]), I64_MAX - int(offsets[-1]) + offsets)):
            field = cc.Field([_compress(timestamps, values, eb)])
            assert np.array_equal(field.ts, timestamps)
            first, last = _span(field)
            for origin, width, n in ((I64_MIN, 50, 700), (first, INTERVAL, 300), (I64_MAX - 40_000, 37, 1_200),
                                     (first - 3 if first > I64_MIN + 3 else I64_MIN, 70, 450),
                                     (I64_MIN, I64_MAX, 3), (I64_MIN, 1 << 62, 4), (last, 1, 1), (I64_MAX, 1, 1),
                                     (I64_MAX - 1_000, I64_MAX, 2)):
                _check(hip, field, None, 1, origin, width, n, f"ends {base} {origin} {width}")
    # a link from one end of int64 towards the other: t1 - t0 near 2^64 is never linked (the gap exceeds any max_gap),
    # one of 2^63 - 1 is
    far = cc.Field([mdb.SegmentBatch.concat([_compress([I64_MIN], [1.0]), _compress([-1], [2.0]),
                                             _compress([I64_MAX - 1], [4.0])])])
    results = _check(hip, far, None, 1, I64_MIN, 1 << 61, 8, "far apart", max_gap=I64_MAX)
    assert results[LINEAR][0]["count"][0].tolist() == [1] * 8
    assert results[EXACT][0]["count"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    ends = cc.Field([mdb.SegmentBatch.concat([_compress([I64_MIN], [1.0]), _compress([I64_MAX], [2.0])])])
    for origin, width, n in ((I64_MIN, 1 << 61, 8), (I64_MIN, I64_MAX, 3), (-1, 1, 2)):
        results = _check(hip, ends, None, 1, origin, width, n, "the two ends", max_gap=I64_MAX)
        assert int(results[LINEAR][0]["count"].sum()) == (1 if origin == I64_MIN else 0)


def test_slices_of_one_pair(hip, monkeypatch):
    """MDB_AGG_BUCKET_SLICE_PAIRS=1, the smallest the library accepts: every segment's pairs straddle slices. Cells
    with count <= 1 stay byte-identical to the default; the others stay within the tolerance; count never moves."""
    field = small_table()[1]
    first, _ = _span(field)
    args = (first + 2_000, 450, 60)
    for groups, n_groups in ((None, 1), (field.groups, 4)):
        for method, name in METHODS:
            whole = hip.sample_at(field.batch, *args, groups=groups, method=method, n_groups=n_groups)
            monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "1")
            sliced = hip.sample_at(field.batch, *args, groups=groups, method=method, n_groups=n_groups)
            monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "7")
            sevens = hip.sample_at(field.batch, *args, groups=groups, method=method, n_groups=n_groups)
            monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
            expected = sc.oracle(field, groups, n_groups, *args, method)
            for cells, what in ((sliced, "1"), (sevens, "7")):
                sc.assert_cells(cells, expected, f"slices of {what} {name} {n_groups} group(s)")
                np.testing.assert_array_equal(cells["count"], whole["count"])
                single = whole["count"] <= 1
                assert cells[single].tobytes() == whole[single].tobytes()
            if groups is None and method != EXACT:
                assert (whole["count"] > 1).any() and (whole["count"] == 1).any()


def test_forms_and_runs_agree_and_cells_are_merged_into(hip):
    field = small_table()[1]
    batch, groups = field.batch, field.groups
    first, _ = _span(field)
    args = (first - 777, 130, 700)
    resident = field.resident(hip)
    cuts = [0, len(batch) // 5, len(batch) // 2, len(batch) - 3, len(batch)]   # (cuts inside series: links cross them)
    assert all(groups[c - 1] == groups[c] for c in cuts[1:-1])
    rng = np.random.default_rng(12)
    for method, name in METHODS:
        expected = sc.oracle(field, groups, 4, *args, method)
        once = hip.sample_at(batch, *args, groups=groups, method=method, n_groups=4)
        sc.assert_cells(once, expected, f"host form {name}")
        assert hip.sample_at(batch, *args, groups=groups, method=method, n_groups=4).tobytes() == once.tobytes()
        assert hip.sample_at_list([batch], *args, groups=[groups], method=method, n_groups=4).tobytes() == once.tobytes()
        on_device = hip.sample_at_dev(resident, *args, groups=groups, method=method, n_groups=4)
        assert on_device.tobytes() == once.tobytes()
        assert hip.sample_at_dev(resident, *args, groups=groups, method=method, n_groups=4).tobytes() == once.tobytes()
        listed = hip.sample_at_list([batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])], *args,
                                    groups=[groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])], method=method, n_groups=4)
        assert listed.tobytes() == once.tobytes()
        # a merge into cells that are not fresh equals fresh cells plus sample_merge
        used = mdb.fresh_sample_cells(once.shape)
        taken = rng.random(once.shape) < 0.5
        used["count"][taken] = rng.integers(1, 9, int(taken.sum()))
        used["sum"][taken] = rng.normal(0.0, 100.0, int(taken.sum()))
        by_hand = mdb.sample_merge(used.copy(), once)
        assert hip.sample_at(batch, *args, groups=groups, method=method, cells=used.copy()).tobytes() == by_hand.tobytes()
        assert hip.sample_at_dev(resident, *args, groups=groups, method=method, cells=used.copy()).tobytes() == by_hand.tobytes()
        # the origin moved back by three widths with three more instants: the cells that still exist, same bytes
        there = hip.sample_at(batch, args[0] - 3 * args[1], args[1], args[2] + 3, groups=groups, method=method, n_groups=4)
        assert np.ascontiguousarray(there[:, 3:]).tobytes() == once.tobytes()
        # the segments in another order: count the same, sum within the tolerance
        order = np.random.default_rng(6).permutation(len(batch))
        shuffled = cc.Field([batch.take(order)])
        moved = hip.sample_at(shuffled.batch, *args, groups=groups[order], method=method, n_groups=4)
        sc.assert_cells(moved, sc.oracle(shuffled, groups[order], 4, *args, method), f"shuffled {name}")


def test_a_resident_batch_keeps_nothing_of_the_operator(hip):
    field = small_table()[2]
    first, _ = _span(field)
    args = (first - 10, 90, 1_000)
    resident = hip.upload_segments(field.batch)
    before = [hip.sample_at_dev(resident, *args, groups=field.groups, method=method, n_groups=4) for method, _ in METHODS]
    timestamps, values = hip.grid_resident(resident)
    assert np.array_equal(timestamps, field.ts) and values.tobytes() == field.values.tobytes()
    hip.integral_buckets_dev(resident, *args, groups=field.groups, n_groups=4)
    timestamps, _ = hip.grid_resident(resident)
    assert np.array_equal(timestamps, field.ts)
    after = [hip.sample_at_dev(resident, *args, groups=field.groups, method=method, n_groups=4) for method, _ in METHODS]
    for one, other, (method, name) in zip(before, after, METHODS):
        assert one.tobytes() == other.tobytes(), name
        sc.assert_cells(one, sc.oracle(field, field.groups, 4, *args, method), f"resident {name}")
    resident.free()


def test_errors_on_the_device_path_leave_the_cells_untouched(hip):
    field = small_table()[1]
    batch, groups = field.parts[0], np.arange(len(field.parts[0]), dtype=np.uint32) % 3
    rng = np.random.default_rng(9)
    cells = np.frombuffer(rng.bytes(3 * 10 * CELL.itemsize), dtype=CELL).reshape(3, 10).copy()
    before = cells.copy()
    resident = hip.upload_segments(batch)
    # a group id out of range, on a row outside every instant
    bad = groups.copy()
    bad[-1] = 3
    assert int(batch.start_time[-1]) > 10 * 1000 and int(batch.start_time[0]) < 10 * 1000
    for call in (lambda: hip.sample_at(batch, 0, 1000, 10, groups=bad, cells=cells, n_groups=3),
                 lambda: hip.sample_at_list([batch.slice(0, 2), batch.slice(2, len(batch))], 0, 1000, 10,
                                            groups=[bad[:2], bad[2:]], cells=cells, n_groups=3),
                 lambda: hip.sample_at_dev(resident, 0, 1000, 10, groups=bad, cells=cells, n_groups=3)):
        with pytest.raises(mdb.HipError, match="group id"):
            call()
        assert cells.tobytes() == before.tobytes()
    # a malformed segment among those the request reaches: a row of a model type that does not exist
    rows = batch.rows()
    rows[len(rows) // 2] = (_abi.MDB_MACAQUE_V_ID + 1,) + rows[len(rows) // 2][1:]
    broken = mdb.SegmentBatch.from_rows(rows)
    origin = int(batch.start_time.min())
    width = (int(batch.end_time.max()) - origin) // 10 + 1
    broken_resident = hip.upload_segments(broken)
    for method, _ in METHODS:
        for call in (lambda: hip.sample_at(broken, origin, width // 7, 70, groups=groups, method=method, cells=cells7),
                     lambda: hip.sample_at_dev(broken_resident, origin, width // 7, 70, groups=groups, method=method,
                                               cells=cells7)):
            cells7 = np.frombuffer(rng.bytes(3 * 70 * CELL.itemsize), dtype=CELL).reshape(3, 70).copy()
            before7 = cells7.copy()
            with pytest.raises(mdb.HipError, match="model type"):
                call()
            assert cells7.tobytes() == before7.tobytes()
    broken_resident.free()
    # the request's own errors reach the device forms too, before `data` (a host pointer here) is touched
    request = hip._sample_request(0, 100, 10, 3, 7, None)
    data = cells.ctypes.data_as(ctypes.c_void_p)
    assert hip.lib.mdb_sample_at_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(request), data) == 1
    assert b"method" in hip.lib.mdb_last_error()
    assert cells.tobytes() == before.tobytes()
    # an empty batch and zero instants succeed and change nothing
    hip.sample_at(batch.slice(0, 0), 0, 100, 10, cells=cells, n_groups=3)
    hip.sample_at_list([], 0, 100, 10, cells=cells, n_groups=3)
    assert cells.tobytes() == before.tobytes()
    none = np.zeros((3, 0), dtype=CELL)
    assert hip.sample_at(batch, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    assert hip.sample_at_dev(resident, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    resident.free()


def test_integral_durations_cover_the_defined_instants(hip):
    """A consistency check with the sibling operator: on fields with no gap, a bucket request and a sample request of
    one origin and width. A bucket with duration > 0 has a defined instant at one of its two edges under STEP."""
    for f in (0, 1, 2):
        for k in (0, 1, 2):
            field = cc.Field([small_table()[f].parts[k]])
            first, last = _span(field)
            for origin, width in ((first, INTERVAL), (first - 30, 70), (first - 1_000, 450), (first + 333, 1_234)):
                n = (last - origin) // width + 3
                durations = hip.integral_buckets(field.batch, origin, width, n, method=mdb.MDB_INTEGRAL_STEP)["duration"][0]
                counts = hip.sample_at(field.batch, origin, width, n + 1, method=STEP)["count"][0]
                defined = counts > 0
                at = origin + width * np.arange(n + 1)
                np.testing.assert_array_equal(defined, (at >= first) & (at <= last))
                assert (durations > 0).any()
                assert (defined[:-1] | defined[1:])[durations > 0].all()


def test_pairing_two_fields_of_different_sampling(hip):
    """The worked example of INTEGRATION.md: wind speed at one rate, power at a tenth of it, brought to one time axis by
    two sample_at calls under LINEAR; the host correlates the two value arrays."""
    n_fast = 3_000
    fast_ts = 50_000 + np.arange(n_fast, dtype=np.int64) * INTERVAL
    slow_ts = 50_370 + np.arange(n_fast // 10, dtype=np.int64) * (10 * INTERVAL)
    wind = datagen.sine_series(3, n_fast)[1]
    power = (0.5 * np.interp(slow_ts, fast_ts, wind.astype(np.float64)) ** 2
             + np.random.default_rng(4).normal(0.0, 5.0, len(slow_ts))).astype(np.float32)
    eb = cases.error_bounds()["rel1"]
    fields = [cc.Field([_compress(fast_ts, wind, eb)]), cc.Field([_compress(slow_ts, power, eb)])]
    origin, width = 50_000, 250
    n = (int(fast_ts[-1]) - origin) // width + 1
    sampled, reference = [], []
    for field in fields:
        cells = hip.sample_at(field.batch, origin, width, n, method=LINEAR)
        expected = sc.oracle(field, None, 1, origin, width, n, LINEAR)
        sc.assert_cells(cells, expected, "pairing")
        sampled.append(mdb.sample_values(cells)[0])
        reference.append(sc.values_of(expected)[0])
    both = ~np.isnan(sampled[0]) & ~np.isnan(sampled[1])
    assert np.array_equal(both, ~np.isnan(reference[0]) & ~np.isnan(reference[1]))
    assert 1_000 < both.sum() < n   # (the slow field begins later and ends earlier: its gaps stay gaps)
    got = np.corrcoef(sampled[0][both], sampled[1][both])[0, 1]
    wanted = np.corrcoef(reference[0][both], reference[1][both])[0, 1]
    print(f"pairing: {int(both.sum())} instants, correlation {got:.12f} (reference {wanted:.12f})")
    assert abs(got - wanted) <= 1e-9 and abs(got) > 0.1
