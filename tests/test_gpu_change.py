"""Changes between consecutive points per date_bin bucket on segments (mdb_change_buckets*): per bucket and group the
linked pairs whose later row lies in the bucket - count, falls, duration, the sums of the rises, of the falls and of the
values after a fall, the largest rise and fall. The tables are tests/comoments_cases.py's; the reference
(tests/change_cases.py) applies the linked rule to the oracle's grid row by row, assigns every pair to the bucket of
its later row in Python integers and sums each cell's terms with math.fsum.

Tolerances are the contract's: count, n_fall, duration, max_rise and max_fall equal in every cell; each of rise, fall
and reset_sum within count * 2^-52 * S of the reference, S the sum of the magnitudes of its terms; rise and fall NaN
exactly in the cells with a NaN difference. Expected values never come from the library under test, except in the test
that says it is a consistency check."""

import ctypes

import numpy as np
import pytest

import cases
import change_cases as chc
import comoments_cases as cc
import datagen
import layouts
import oracle_lib as ora
import scale_cases as scale
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
CELL = mdb.CHANGE_CELL_DTYPE
VALUE_MEMBERS = ("rise", "fall", "reset_sum", "max_rise", "max_fall")
EDGE_EPOCH = 1658671178037  # the first timestamp of the edge cases' epoch-scale series
SLICE_SWITCH = b"MDB_AGG_BUCKET_SLICE_PAIRS"


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()


def _span(field):
    return int(field.ts.min()), int(field.ts.max())


def _compress(timestamps, values, eb=cases.LOSSLESS):
    return ora.try_compress_univariate_time_series(np.asarray(timestamps, dtype=np.int64),
                                                   np.asarray(values, dtype=np.float32), eb)


def _fresh(cells):
    return cells.tobytes() == bytes(cells.size * CELL.itemsize)


@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "one_group"])
@pytest.mark.parametrize("f", [0, 1, 2], ids=["lossless", "rel1", "abs5"])
def test_parity_with_the_rows_in_exact_arithmetic(hip, f, grouped):
    """All three model types, regular and irregular timestamps, residual tails, segments far longer and far shorter
    than 64 rows; every bucket set of comoments_cases with its time range dropped; every cell compared."""
    field = cc.main_table()[f]
    assert np.isfinite(field.values).all()
    groups, n_groups = (field.groups, 4) if grouped else (None, 1)
    for name, origin, width, n_buckets, _, _ in cc.bucket_sets(*_span(field)):
        got = hip.change_buckets(field.batch, origin, width, n_buckets, groups=groups, n_groups=n_groups)
        expected = chc.oracle(field, groups, n_groups, origin, width, n_buckets)
        _, poisoned = chc.assert_cells(got, expected, f"field {f} {name} {n_groups} group(s)")
        assert poisoned == 0


@pytest.mark.parametrize("f", [0, 1], ids=["lossless", "abs5"])
def test_non_finite_values(hip, f):
    """NaN, +-0, +-inf, one- and two-point segments, epoch-scale Swing, width 2^40: each series a group. A poisoned
    cell has NaN rise and fall and exact count, n_fall, duration and maxima."""
    field = cc.edge_table()[f]
    n_groups = len(field.parts)
    plain = poisoned = 0
    for origin, width, n_buckets in ((0, 100, 40), (-35, 250, 24), (EDGE_EPOCH - 1000, 3000, 30),
                                     (EDGE_EPOCH, 50_000, 10), (0, 1 << 40, 3)):
        got = hip.change_buckets(field.batch, origin, width, n_buckets, groups=field.groups, n_groups=n_groups)
        counts = chc.assert_cells(got, chc.oracle(field, field.groups, n_groups, origin, width, n_buckets),
                                  f"edge {origin} {width}")
        plain, poisoned = plain + counts[0], poisoned + counts[1]
    assert plain > 0 and poisoned > 0   # (both kinds of cell were among them)


def test_a_link_across_many_buckets(hip):
    """Two one-point segments, (0, 1.0) and (10 000, 3.0): the only pair is the link between them, and it belongs to
    the bucket of its later row whole. Width 100: at origin 0 with 101 buckets only bucket 100 is touched; at origin
    50 with 99 buckets (they end at 9 950) the pair is dropped."""
    field = cc.Field([_compress([0], [1.0]), _compress([10_000], [3.0])])
    assert len(field.batch) == 2 and field.ts.tolist() == [0, 10_000] and field.values.tolist() == [1.0, 3.0]
    got = hip.change_buckets(field.batch, 0, 100, 101)
    chc.assert_cells(got, chc.oracle(field, None, 1, 0, 100, 101), "link, origin 0")
    assert _fresh(got[0, :100])
    assert got[0, 100].tolist() == (1, 0, 10_000, 2.0, 0.0, 0.0, 2.0, 0.0)
    assert _fresh(hip.change_buckets(field.batch, 50, 100, 99))
    # the earlier row may lie before the origin: at origin 9 950 the pair is in bucket 0
    assert hip.change_buckets(field.batch, 9_950, 100, 2)[0, 0].tolist() == (1, 0, 10_000, 2.0, 0.0, 0.0, 2.0, 0.0)


def test_short_segments(hip):
    """Series 3 of the main table (runs of 2..12 points) alone, under every error bound; and 600 irregular points cut
    into segments of 1..5 points: as many links between segments as pairs inside them. Every row but the first is the
    later row of one pair."""
    for f in (0, 1, 2):
        field = cc.Field([cc.main_table()[f].parts[3]])
        first, last = _span(field)
        assert len(field.ts) == 1500 and len(field.batch) >= 6
        for origin, width, n_buckets in ((first, last - first + 1, 1), (first, INTERVAL, (last - first) // INTERVAL + 1)):
            got = hip.change_buckets(field.batch, origin, width, n_buckets)
            chc.assert_cells(got, chc.oracle(field, None, 1, origin, width, n_buckets), f"short {f} {width}")
            assert int(got["count"].sum()) == len(field.ts) - 1 and int(got["duration"].sum()) == last - first
            if width == INTERVAL:
                assert got["count"][0, 0] == 0 and (got["count"][0, 1:] == 1).all()
    rng = np.random.default_rng(5)
    n = 600
    timestamps = 1_000 + np.cumsum(rng.integers(1, 400, n))
    values = datagen.sine_series(9, n)[1]
    cuts = np.concatenate([[0], np.minimum(np.cumsum(rng.integers(1, 6, n)), n)])
    cuts = cuts[:int(np.argmax(cuts == n)) + 1]
    tiny = cc.Field([_compress(timestamps[a:b], values[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(tiny.ts, timestamps) and len(tiny.batch) > n // 5
    first, last = _span(tiny)
    for origin, width, n_buckets in ((first - 55, 170, (last - first) // 170 + 2), (first, last - first + 1, 1)):
        got = hip.change_buckets(tiny.batch, origin, width, n_buckets)
        chc.assert_cells(got, chc.oracle(tiny, None, 1, origin, width, n_buckets), f"tiny {width}")
        assert int(got["count"].sum()) == n - 1 and int(got["duration"].sum()) == last - first


def test_the_gap_rule(hip):
    field = cc.Field([cc.main_table()[0].parts[0]])   # regular, lossless
    first, last = _span(field)
    assert (np.diff(field.ts) == INTERVAL).all()
    args = (first - 30, 7 * INTERVAL, (last - first) // (7 * INTERVAL) + 2)
    assert _fresh(hip.change_buckets(field.batch, *args, max_gap=INTERVAL - 1))
    assert _fresh(hip.change_buckets(field.batch, *args, max_gap=0))
    equal = hip.change_buckets(field.batch, *args, max_gap=INTERVAL)
    chc.assert_cells(equal, chc.oracle(field, None, 1, *args, INTERVAL), "gap equal")
    assert int(equal["count"].sum()) == len(field.ts) - 1 and int(equal["duration"].sum()) == last - first
    assert equal.tobytes() == hip.change_buckets(field.batch, *args).tobytes()
    # the same under a lossy bound: PMC-Mean and Swing rows, whose sampling interval the rule sees too
    lossy = cc.Field([cc.main_table()[2].parts[0]])
    assert _fresh(hip.change_buckets(lossy.batch, *args, max_gap=INTERVAL - 1))
    chc.assert_cells(hip.change_buckets(lossy.batch, *args, max_gap=INTERVAL),
                     chc.oracle(lossy, None, 1, *args, INTERVAL), "gap equal, lossy")


def test_what_is_not_linked(hip):
    main = cc.main_table()[1]
    # a step back in time (the series boundaries of the main table) with groups=None: no link crosses them
    first, last = _span(main)
    series_rows = [int((main.groups[main.segment] == k).sum()) for k in range(4)]
    got = hip.change_buckets(main.batch, first, last - first + 1, 1)
    chc.assert_cells(got, chc.oracle(main, None, 1, first, last - first + 1, 1), "boundaries")
    assert int(got["count"][0, 0]) == sum(series_rows) - 4
    # a group change in the middle of a series: the pair between the two segments is lost, nothing else
    series = cc.Field([main.parts[0]])
    first, last = _span(series)
    cut = len(series.batch) // 2
    groups = (np.arange(len(series.batch)) >= cut).astype(np.uint32)
    rows_before = int(series.rows[:cut].sum())
    args = (first, 50 * INTERVAL, (last - first) // (50 * INTERVAL) + 1)
    got = hip.change_buckets(series.batch, *args, groups=groups, n_groups=2)
    chc.assert_cells(got, chc.oracle(series, groups, 2, *args), "group change")
    assert int(got["count"][0].sum()) == rows_before - 1 and int(got["count"][1].sum()) == len(series.ts) - rows_before - 1
    # time standing still: (500, 1) and (500, 2) are not linked; (500, 2) and (600, 4) are
    equal = cc.Field([_compress([500], [1.0]), _compress([500], [2.0]), _compress([600], [4.0])])
    assert equal.ts.tolist() == [500, 500, 600]
    got = hip.change_buckets(equal.batch, 0, 1_000, 1)
    chc.assert_cells(got, chc.oracle(equal, None, 1, 0, 1_000, 1), "equal timestamps")
    assert got[0, 0].tolist() == (1, 0, 100, 2.0, 0.0, 0.0, 2.0, 0.0)
    # a segment with end_time < start_time in between rebuilds to no row and links nothing across it
    # (the rows 200 and 500 are consecutive rows of the grid, so the expected cell is written out by hand)
    left, right = _compress([100, 200], [1.0, 2.0]).rows(), _compress([500, 600], [2.0, 7.0]).rows()
    broken = mdb.SegmentBatch.from_rows(left + [(0, 400, 300, bytes([5]), 9.0, 9.0, b"", b"")] + right)
    timestamps, _, per_segment, _ = ora.grid_batch(broken)
    assert timestamps.tolist() == [100, 200, 500, 600] and per_segment.tolist()[len(left)] == 0
    got = hip.change_buckets(broken, 0, 1_000, 1)
    assert got[0, 0].tolist() == (2, 0, 200, 6.0, 0.0, 0.0, 5.0, 0.0)
    whole = mdb.SegmentBatch.from_rows(left + right)   # without it the two are linked: 200 -> 500, 2.0 -> 2.0
    assert hip.change_buckets(whole, 0, 1_000, 1)[0, 0].tolist() == (3, 0, 500, 6.0, 0.0, 0.0, 5.0, 0.0)


def test_constant_series_and_pmc_mean_in_closed_form(hip):
    """Levels held for 500 points each (PMC-Mean runs): inside a run every difference is zero. And one level in
    PMC-Mean segments of 7 and of 5 000 rows: count and duration from row indices, the five value members exactly 0."""
    steps = cc.steps_table()[0]
    assert (steps.batch.model_type_id == mdb.MDB_PMC_MEAN_ID).all() and len(steps.batch) >= 12
    for intervals in (500, 250, 100):
        width, n_buckets = intervals * INTERVAL, 6000 // intervals
        got = hip.change_buckets(steps.batch, 0, width, n_buckets)
        chc.assert_cells(got, chc.oracle(steps, None, 1, 0, width, n_buckets), f"levels {intervals}")
        inside = np.arange(n_buckets) % (500 // intervals) != 0   # (no run begins in these buckets)
        assert inside.any() or intervals == 500
        for member in VALUE_MEMBERS:
            assert (got[member][0, inside] == 0.0).all() and not np.signbit(got[member][0, inside]).any()
    lengths = np.array([7, 5_000, 7, 5_000, 5_000, 7, 7], dtype=np.int64)
    delta = 10
    starts = 1_000 + delta * np.concatenate([[0], np.cumsum(lengths)[:-1]])
    level = np.full(len(lengths), 21.5, dtype=np.float32)
    batch = scale.simple_batch(np.full(len(lengths), scale.PMC), starts, lengths, np.full(len(lengths), delta), level,
                               level, np.zeros(len(lengths), dtype=bool))
    n_rows = int(lengths.sum())
    for origin, width in ((1_000, 640), (777, 12_345), (1_000, delta), (0, 10 * n_rows * delta)):
        n_buckets = (1_000 + n_rows * delta - origin) // width + 2
        got = hip.change_buckets(batch, origin, width, n_buckets)
        later = 1_000 + delta * np.arange(1, n_rows)   # the later row of every pair
        count = np.bincount((later - origin) // width, minlength=n_buckets)
        np.testing.assert_array_equal(got["count"][0], count)
        np.testing.assert_array_equal(got["duration"][0], count * delta)
        np.testing.assert_array_equal(got["n_fall"][0], 0)
        for member in VALUE_MEMBERS:
            assert got[member].tobytes() == bytes(8 * n_buckets), member
    # each segment a group of its own: nothing links them
    groups = np.arange(len(lengths), dtype=np.uint32)
    alone = hip.change_buckets(batch, 0, 10 * n_rows * delta, 1, groups=groups)
    np.testing.assert_array_equal(alone["count"][:, 0], lengths - 1)
    np.testing.assert_array_equal(alone["duration"][:, 0], (lengths - 1) * delta)


def test_a_counter_with_restarts(hip):
    """Integer-valued float32 values rising by 0..3 per row, restarted to a small integer every 97 rows, lossless;
    buckets of 250 rows. Every sum is an integer below 2^24, so every member is exact; the increase and the restarts
    per bucket are the generator's own."""
    rng = np.random.default_rng(41)
    n, every, per_bucket = 3_000, 97, 250
    counter = np.zeros(n, dtype=np.int64)
    counter[0] = 10
    restarts = np.zeros(n, dtype=bool)
    for k in range(1, n):
        restarts[k] = k % every == 0
        counter[k] = int(rng.integers(0, 6)) if restarts[k] else counter[k - 1] + int(rng.integers(0, 4))
    assert (counter[restarts] < counter[np.nonzero(restarts)[0] - 1]).all() and counter.max() < 1 << 12
    timestamps = 50_000 + INTERVAL * np.arange(n, dtype=np.int64)
    field = cc.Field([_compress(timestamps, counter.astype(np.float32))])
    assert np.array_equal(field.ts, timestamps) and np.array_equal(field.values, counter.astype(np.float32))
    n_buckets = n // per_bucket
    got = hip.change_buckets(field.batch, 50_000, per_bucket * INTERVAL, n_buckets)
    bucket = np.arange(1, n) // per_bucket             # of the later row of pair (k - 1, k)
    step = np.diff(counter)
    reset = restarts[1:]
    assert ((step < 0) == reset).all()
    total = lambda terms: np.bincount(bucket, weights=terms, minlength=n_buckets)
    expected = np.zeros((1, n_buckets), dtype=CELL)
    expected["count"][0] = np.bincount(bucket, minlength=n_buckets)
    expected["n_fall"][0] = total(reset)
    expected["duration"][0] = expected["count"][0] * INTERVAL
    expected["rise"][0] = total(np.where(step > 0, step, 0))
    expected["fall"][0] = total(np.where(reset, -step, 0))
    expected["reset_sum"][0] = total(np.where(reset, counter[1:], 0))
    for b in range(n_buckets):
        expected["max_rise"][0, b] = np.where(step > 0, step, 0)[bucket == b].max()
        expected["max_fall"][0, b] = np.where(reset, -step, 0)[bucket == b].max()
    for member in CELL.names:
        np.testing.assert_array_equal(got[member], expected[member], err_msg=member)
    chc.assert_cells(got, chc.oracle(field, None, 1, 50_000, per_bucket * INTERVAL, n_buckets), "counter")
    np.testing.assert_array_equal(mdb.change_finish(got, mdb.MDB_CHANGE_INCREASE)[0],
                                  total(np.where(reset, counter[1:], step)))
    np.testing.assert_array_equal(got["n_fall"][0], total(reset).astype(np.uint64))
    assert got["n_fall"].sum() == (n - 1) // every
    rate = mdb.change_finish(got, mdb.MDB_CHANGE_RATE)[0]
    np.testing.assert_array_equal(rate, total(np.where(reset, counter[1:], step)) * 1e6 / (expected["count"][0] * INTERVAL))


def test_swing_only(hip):
    """Swing segments alone (ramps up, down and flat; 2 .. 700 rows): the rows are arithmetic in registers. The values
    of a segment are monotone, so a rising one has no fall and a falling one falls on every row that is not flat;
    n_fall and the maxima are bit-equal to the reference's."""
    lengths = np.array([2, 3, 64, 65, 700, 129, 2, 300], dtype=np.int64)
    first = np.array([1.0, 5.0, -3.0, 100.0, 0.125, 7.0, 2.0, 1e-3], dtype=np.float32)
    last = np.array([2.0, 5.5, 40.0, 100.5, 900.0, 7.0, 9.0, 2e-3], dtype=np.float32)
    decreasing = np.array([False, True, False, True, True, False, True, False])
    delta = 100
    starts = 3_000 + delta * np.concatenate([[0], np.cumsum(lengths)[:-1]])
    batch = scale.simple_batch(np.full(len(lengths), scale.SWING), starts, lengths, np.full(len(lengths), delta), first,
                               last, decreasing)
    assert (batch.model_type_id == mdb.MDB_SWING_ID).all()
    field = cc.Field([batch])
    assert len(field.ts) == int(lengths.sum()) and (np.diff(field.ts) == delta).all()
    groups = np.arange(len(lengths), dtype=np.uint32)
    span = int(field.ts[-1]) - 3_000
    for origin, width in ((3_000, delta), (2_950, 7 * delta), (3_000 - 12_345, 3_333), (3_000, span + 1)):
        n_buckets = (int(field.ts[-1]) - origin) // width + 2
        got = hip.change_buckets(field.batch, origin, width, n_buckets)
        chc.assert_cells(got, chc.oracle(field, None, 1, origin, width, n_buckets), f"swing {width}")
        alone = hip.change_buckets(field.batch, origin, width, n_buckets, groups=groups)
        expected = chc.oracle(field, groups, len(lengths), origin, width, n_buckets)
        chc.assert_cells(alone, expected, f"swing {width}, each segment a group")
        for k in range(len(lengths)):
            values = field.values[field.segment == k].astype(np.float64)
            flat = int((np.diff(values) == 0).sum())
            pairs, falls = int(alone["count"][k].sum()), int(alone["n_fall"][k].sum())
            assert pairs == lengths[k] - 1
            assert falls == (pairs - flat if decreasing[k] and first[k] != last[k] else 0), k
            if falls == 0:
                assert (alone["fall"][k] == 0.0).all() and (alone["max_fall"][k] == 0.0).all()
            for member in ("max_rise", "max_fall"):
                assert alone[member][k].tobytes() == expected[member][k].tobytes()


def test_adjacent_buckets_add_up(hip):
    field = cc.main_table()[2]
    first, last = _span(field)
    for width in (3 * INTERVAL, 3_333):
        origin, n_wide = first - 12_345, (last - first + 12_345) // (2 * width) + 2
        narrow = hip.change_buckets(field.batch, origin, width, 2 * n_wide, groups=field.groups, n_groups=4)
        wide = hip.change_buckets(field.batch, origin, 2 * width, n_wide, groups=field.groups, n_groups=4)
        expected = chc.oracle(field, field.groups, 4, origin, 2 * width, n_wide)
        chc.assert_cells(wide, expected, f"wide {width}")
        folded = mdb.change_merge(np.ascontiguousarray(narrow[:, 0::2]), np.ascontiguousarray(narrow[:, 1::2]))
        chc.assert_cells(folded, expected, f"narrow pairs merged {width}")
        for member in chc.EXACT:
            np.testing.assert_array_equal(folded[member], wide[member], err_msg=member)


def test_durations_agree_with_the_time_weighted_operator(hip):
    """A consistency check with an independent operator: with buckets that cover every row, both operators see the
    same linked pairs, so the durations add up to the same linked time under every gap rule."""
    field = cc.main_table()[1]
    first, last = _span(field)
    args = (first - 500, 12_345, (last - first + 500) // 12_345 + 2)
    for max_gap in (INTERVAL, 3 * INTERVAL, None):
        change = hip.change_buckets(field.batch, *args, groups=field.groups, max_gap=max_gap, n_groups=4)
        integral = hip.integral_buckets(field.batch, *args, groups=field.groups, max_gap=max_gap, n_groups=4)
        assert int(change["duration"].sum()) == int(integral["duration"].sum()) > 0
        np.testing.assert_array_equal(change["duration"].sum(axis=1), integral["duration"].sum(axis=1))


def test_forms_runs_and_placement(hip):
    field = cc.main_table()[1]
    batch, groups = field.batch, field.groups
    lowest = int(field.ts.min())
    args = (lowest - 777 - 3 * 1_300, 1_300, 1_003)   # (buckets 0, 1 and 2 lie before all data)
    resident = field.resident(hip)
    cuts = [0, len(batch) // 5, len(batch) // 2, len(batch) - 7, len(batch)]   # (cuts inside series: links cross them)
    assert all(groups[c - 1] == groups[c] for c in cuts[1:-1])
    pairs = np.unique(field.segment * args[2] + (field.ts - args[0]) // args[1])   # (segment, bucket), oracle alone
    assert len(pairs) > 1_000
    expected = chc.oracle(field, groups, 4, *args)
    first = hip.change_buckets(batch, *args, groups=groups, n_groups=4)
    chc.assert_cells(first, expected, "host form")
    assert hip.change_buckets(batch, *args, groups=groups, n_groups=4).tobytes() == first.tobytes()
    assert hip.change_buckets_list([batch], *args, groups=[groups], n_groups=4).tobytes() == first.tobytes()
    assert hip.change_buckets_dev(resident, *args, groups=groups, n_groups=4).tobytes() == first.tobytes()
    assert hip.change_buckets_dev(resident, *args, groups=groups, n_groups=4).tobytes() == first.tobytes()
    listed = hip.change_buckets_list([batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])], *args,
                                     groups=[groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])], n_groups=4)
    assert listed.tobytes() == first.tobytes()
    # the origin moved by three widths either way, n_buckets moved along: the cells that still exist, same bytes
    back = hip.change_buckets(batch, args[0] - 3 * args[1], args[1], args[2] + 3, groups=groups, n_groups=4)
    assert _fresh(back[:, :3]) and np.ascontiguousarray(back[:, 3:]).tobytes() == first.tobytes()
    forward = hip.change_buckets(batch, args[0] + 3 * args[1], args[1], args[2] - 3, groups=groups, n_groups=4)
    assert _fresh(first[:, :3]) and forward.tobytes() == np.ascontiguousarray(first[:, 3:]).tobytes()
    # ... and moved forward over buckets that hold rows: those pairs leave, so the runs of the reduction are cut
    # elsewhere - the exact members of the cells that remain keep their bytes, the sums move by rounding only
    beyond = hip.change_buckets(batch, args[0] + 50 * args[1], args[1], args[2] - 50, groups=groups, n_groups=4)
    assert not _fresh(first[:, 3:50])
    chc.assert_cells(beyond, chc.oracle(field, groups, 4, args[0] + 50 * args[1], args[1], args[2] - 50), "origin moved over rows")
    for member in chc.EXACT:
        np.testing.assert_array_equal(beyond[member], first[member][:, 50:], err_msg=member)
    # slices of 64 and of 1 000 pairs: the exact members equal, the sums within the tolerance
    reloading = _abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL
    try:
        _abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL = False   # (a reload would put the environment's value back)
        for pairs_per_slice in (b"64", b"1000"):
            assert hip.lib.mdb_set_option(SLICE_SWITCH, pairs_per_slice) == 0
            sliced = hip.change_buckets(batch, *args, groups=groups, n_groups=4)
            on_device = hip.change_buckets_dev(resident, *args, groups=groups, n_groups=4)
            one = hip.change_buckets(batch, args[0], args[1] * args[2], 1, groups=groups, n_groups=4)
            assert hip.lib.mdb_option(SLICE_SWITCH) == pairs_per_slice
            chc.assert_cells(sliced, expected, f"slices of {int(pairs_per_slice)} pairs")
            assert on_device.tobytes() == sliced.tobytes()
            for member in chc.EXACT:
                np.testing.assert_array_equal(sliced[member], first[member], err_msg=member)
            chc.assert_cells(one, chc.oracle(field, groups, 4, args[0], args[1] * args[2], 1),
                             f"slices of {int(pairs_per_slice)} pairs, one bucket")
    finally:
        hip.lib.mdb_set_option(SLICE_SWITCH, None)
        _abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL = reloading
    # the segments in another order (the sort path): rounding only
    order = np.random.default_rng(6).permutation(len(batch))
    shuffled = cc.Field([batch.take(order)])
    moved = hip.change_buckets(shuffled.batch, *args, groups=groups[order], n_groups=4)
    chc.assert_cells(moved, chc.oracle(shuffled, groups[order], 4, *args), "shuffled")


def test_merging_into_cells_that_are_not_fresh(hip):
    """Two calls over the two halves of the table, cut at a series boundary (no link crosses it), equal one call."""
    field = cc.main_table()[0]
    batch, groups = field.batch, field.groups
    first, last = _span(field)
    args = (first - 40, 2_900, (last - first + 40) // 2_900 + 1)
    cut = len(field.parts[0]) + len(field.parts[1])
    halves = (batch.slice(0, cut), batch.slice(cut, len(batch)))
    once = hip.change_buckets(batch, *args, groups=groups, n_groups=4)
    cells = hip.change_buckets(halves[0], *args, groups=groups[:cut], n_groups=4)
    assert not _fresh(cells[:2]) and _fresh(cells[2:])
    twice = hip.change_buckets(halves[1], *args, groups=groups[cut:], cells=cells)
    # no cell is shared (each series a group): the first half's cells keep their bytes, and the whole equals one call
    # in the exact members and, the second half's pairs being numbered anew, in the sums up to rounding
    assert twice is cells and twice[:2].tobytes() == once[:2].tobytes()
    chc.assert_cells(twice, chc.oracle(field, groups, 4, *args), "two calls, four groups")
    for member in chc.EXACT:
        np.testing.assert_array_equal(twice[member], once[member], err_msg=member)
    # one group: the series overlap in time, so cells are merged into
    once = hip.change_buckets(batch, *args)
    expected = chc.oracle(field, None, 1, *args)
    chc.assert_cells(once, expected, "one call")
    cells = hip.change_buckets(halves[0], *args)
    second = hip.upload_segments(halves[1])
    twice = hip.change_buckets_dev(second, *args, cells=cells)
    second.free()
    chc.assert_cells(twice, expected, "two calls, one group", fresh=False)
    for member in chc.EXACT:
        np.testing.assert_array_equal(twice[member], once[member], err_msg=member)
    # a second call over everything doubles the integers and the sums (x + x is exact) and keeps the maxima
    again = hip.change_buckets(batch, *args, cells=once.copy())
    for member in ("count", "n_fall", "duration", "rise", "fall", "reset_sum"):
        np.testing.assert_array_equal(again[member], 2 * once[member], err_msg=member)
    assert again["max_rise"].tobytes() == once["max_rise"].tobytes() and again["max_fall"].tobytes() == once["max_fall"].tobytes()
    assert mdb.change_merge(once.copy(), once).tobytes() == again.tobytes()


def test_a_resident_batch_keeps_nothing_of_the_operator(hip):
    field = cc.Field([cc.main_table()[2].parts[1], cc.main_table()[2].parts[3]])
    first, last = _span(field)
    args = (first - 10, 900, (last - first) // 900 + 2)
    resident = hip.upload_segments(field.batch)
    before = hip.change_buckets_dev(resident, *args, groups=field.groups, n_groups=2)
    timestamps, values = hip.grid_resident(resident)
    assert np.array_equal(timestamps, field.ts) and values.tobytes() == field.values.tobytes()
    after = hip.change_buckets_dev(resident, *args, groups=field.groups, n_groups=2)
    assert before.tobytes() == after.tobytes()
    chc.assert_cells(before, chc.oracle(field, field.groups, 2, *args), "resident")
    timestamps, _ = hip.grid_resident(resident)
    assert np.array_equal(timestamps, field.ts)
    resident.free()


_PLAIN = {}


@pytest.mark.parametrize("mode", layouts.MODES)
def test_binary_view_layouts(hip, mode):
    """Multi-buffer and padded BinaryView columns (tests/layouts.py) give the bytes of the plain layout."""
    field = cc.Field([cc.main_table()[1].parts[1]])   # irregular timestamps, all three model types, residual tails
    first, last = _span(field)
    args = (first - 5, 777, (last - first) // 777 + 2)
    if "cells" not in _PLAIN:
        _PLAIN["cells"] = hip.change_buckets(field.batch, *args)
        chc.assert_cells(_PLAIN["cells"], chc.oracle(field, None, 1, *args), "plain layout")
    relaid = layouts.relayout(field.batch, mode, 7)
    assert hip.change_buckets(relaid, *args).tobytes() == _PLAIN["cells"].tobytes()
    parts = layouts.three_parts(field.batch, mode, 7)
    assert hip.change_buckets_list(parts, *args).tobytes() == _PLAIN["cells"].tobytes()


def test_the_convenience_is_one_bucket_over_the_span(hip):
    field = cc.main_table()[0]
    first, last = _span(field)
    cells = hip.change(field.batch, groups=field.groups, n_groups=4, max_gap=INTERVAL)
    assert cells.shape == (4,)
    chc.assert_cells(cells.reshape(4, 1), chc.oracle(field, field.groups, 4, first, last - first + 1, 1, INTERVAL), "change()")
    assert _fresh(hip.change(field.batch.slice(0, 0), n_groups=2))


def test_errors_leave_the_cells_untouched(hip):
    field = cc.main_table()[1]
    batch, groups = field.parts[0], np.arange(len(field.parts[0]), dtype=np.uint32) % 3
    rng = np.random.default_rng(9)
    cells = np.frombuffer(rng.bytes(3 * 10 * CELL.itemsize), dtype=CELL).reshape(3, 10).copy()
    before = cells.copy()
    resident = hip.upload_segments(batch)
    data = cells.ctypes.data_as(ctypes.c_void_p)
    seg = batch.as_c()

    def request(origin=0, width=1000, n_buckets=10, n_groups=3, max_gap=None, **fields):
        q = hip._change_request(origin, width, n_buckets, n_groups, max_gap)
        for name, value in fields.items():
            setattr(q.buckets if name in ("t_lo", "t_hi", "which_mask") else q, name, value)
        return q

    # the request's own errors, in the host form and - before `data` (a host pointer here) is touched - the device form
    for bad, message in ((request(width=0), b"width"), (request(width=-5), b"width"), (request(n_groups=0), b"n_groups"),
                         (request(which_mask=1), b"which_mask"), (request(t_lo=0), b"time range"),
                         (request(t_hi=10**9), b"time range"), (request(reserved=1), b"reserved"),
                         (request(flags=2), b"flags"), (request(max_gap=-1), b"max_gap")):
        for call in (lambda: hip.lib.mdb_change_buckets(hip.handle, ctypes.byref(seg), None, ctypes.byref(bad), data),
                     lambda: hip.lib.mdb_change_buckets_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(bad), data)):
            assert call() == 1
            assert message in hip.lib.mdb_last_error(), message
            assert cells.tobytes() == before.tobytes()
    good = request()
    for arguments in ((None, ctypes.byref(seg), None, ctypes.byref(good), data), (hip.handle, None, None, ctypes.byref(good), data),
                      (hip.handle, ctypes.byref(seg), None, None, data), (hip.handle, ctypes.byref(seg), None, ctypes.byref(good), None)):
        assert hip.lib.mdb_change_buckets(*arguments) == 1 and b"NULL" in hip.lib.mdb_last_error()
    assert cells.tobytes() == before.tobytes()
    # a group id out of range, on a row no bucket reaches
    bad = groups.copy()
    bad[-1] = 3
    assert int(batch.start_time[-1]) > 10 * 1000 and int(batch.start_time[0]) < 10 * 1000
    for call in (lambda: hip.change_buckets(batch, 0, 1000, 10, groups=bad, cells=cells, n_groups=3),
                 lambda: hip.change_buckets_list([batch.slice(0, 5), batch.slice(5, len(batch))], 0, 1000, 10,
                                                 groups=[bad[:5], bad[5:]], cells=cells, n_groups=3),
                 lambda: hip.change_buckets_dev(resident, 0, 1000, 10, groups=bad, cells=cells, n_groups=3)):
        with pytest.raises(mdb.HipError, match="group id"):
            call()
        assert cells.tobytes() == before.tobytes()
    resident.free()
    # a truncated values buffer on a reached segment: five points of MacaqueV values in five bytes
    pmc = lambda start, level: (0, start, start + 400, bytes([5]), level, level, b"", b"")
    truncated = mdb.SegmentBatch.from_rows([pmc(0, 1.5), (2, 500, 900, bytes([5]), 0.0, 0.0, bytes([1, 2, 3, 4, 0]), b""),
                                            pmc(1_000, 2.5)])
    one = np.frombuffer(rng.bytes(20 * CELL.itemsize), dtype=CELL).reshape(1, 20).copy()
    one_before = one.copy()
    truncated_resident = hip.upload_segments(truncated)
    for call in (lambda: hip.change_buckets(truncated, 0, 100, 20, cells=one),
                 lambda: hip.change_buckets_dev(truncated_resident, 0, 100, 20, cells=one)):
        with pytest.raises(mdb.HipError, match="Malformed segment"):
            call()
        assert one.tobytes() == one_before.tobytes()
    truncated_resident.free()
    # ... and on the neighbour whose first point is read, which no bucket reaches itself: the buckets end at 500
    neighbour = mdb.SegmentBatch.from_rows([pmc(0, 1.5), (2, 500, 900, bytes([5]), 0.0, 0.0, b"ab", b"")])
    neighbour_resident = hip.upload_segments(neighbour)
    for call in (lambda: hip.change_buckets(neighbour, 0, 100, 5, cells=one[:, :5].copy()),
                 lambda: hip.change_buckets_dev(neighbour_resident, 0, 100, 5, cells=one[:, :5].copy())):
        with pytest.raises(mdb.HipError, match="Malformed segment"):
            call()
    neighbour_resident.free()
    # the same segments without the broken one are fine: the pair across the hole belongs to the bucket of 1 000
    whole = hip.change_buckets(mdb.SegmentBatch.from_rows([pmc(0, 1.5), pmc(1_000, 2.5)]), 0, 100, 20)
    assert whole["count"][0].tolist() == [0, 1, 1, 1, 1] + [0] * 5 + [1, 1, 1, 1, 1] + [0] * 5
    assert whole[0, 10].tolist() == (1, 0, 600, 1.0, 0.0, 0.0, 1.0, 0.0)


def test_nothing_to_do_succeeds_and_changes_nothing(hip):
    batch = cc.main_table()[1].parts[0]
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    rng = np.random.default_rng(10)
    cells = np.frombuffer(rng.bytes(3 * 10 * CELL.itemsize), dtype=CELL).reshape(3, 10).copy()
    before = cells.copy()
    resident = hip.upload_segments(batch)
    hip.change_buckets(batch.slice(0, 0), 0, 100, 10, cells=cells, n_groups=3)
    hip.change_buckets_list([], 0, 100, 10, cells=cells, n_groups=3)
    hip.change_buckets_list([batch.slice(0, 0), batch.slice(3, 3)], 0, 100, 10, cells=cells, n_groups=3)
    # buckets no row reaches
    hip.change_buckets(batch, int(batch.end_time.max()) + 1, 100, 10, groups=groups, cells=cells)
    hip.change_buckets_dev(resident, -10_000, 100, 10, groups=groups, cells=cells)
    assert cells.tobytes() == before.tobytes()
    none = np.zeros((3, 0), dtype=CELL)
    assert hip.change_buckets(batch, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    assert hip.change_buckets_dev(resident, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    resident.free()
