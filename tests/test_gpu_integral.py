"""Time-weighted averages and integrals per date_bin bucket on segments (mdb_integral_buckets*): per bucket and group
the microseconds on which the series is defined and its integral over them, LINEAR (trapezoid) and STEP (last
observation carried forward). The tables are tests/comoments_cases.py's; the reference (tests/integral_cases.py)
applies the linked rule to the oracle's grid row by row, walks every linked interval over the buckets it crosses in
Python integers and sums each cell's pieces with math.fsum.

Tolerances are the contract's: duration equal in every cell; |integral - reference| <= 1e-5 * sum (e - a) *
max(|v0|, |v1|) over the cell's pieces; a cell filled by one finite level c has an average within 2^-44 |c| of c; a
cell with a non-finite value that its method reads has a non-finite integral and an exact duration. Expected values
never come from the library under test, except in the tests that say they are consistency checks."""

import ctypes

import numpy as np
import pytest

import cases
import comoments_cases as cc
import datagen
import integral_cases as ic
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
CELL = mdb.INTEGRAL_CELL_DTYPE
LINEAR, STEP = mdb.MDB_INTEGRAL_LINEAR, mdb.MDB_INTEGRAL_STEP
METHODS = ((LINEAR, "linear"), (STEP, "step"))
EDGE_EPOCH = 1658671178037  # the first timestamp of the edge cases' epoch-scale series


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()


def _span(field):
    return int(field.ts.min()), int(field.ts.max())


def _compress(timestamps, values):
    return ora.try_compress_univariate_time_series(np.asarray(timestamps, dtype=np.int64),
                                                   np.asarray(values, dtype=np.float32), cases.LOSSLESS)


@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "one_group"])
@pytest.mark.parametrize("f", [0, 1, 2], ids=["lossless", "rel1", "abs5"])
def test_parity_with_the_rows_in_exact_arithmetic(hip, f, grouped):
    """All three model types, regular and irregular timestamps, segments far longer and far shorter than 64 rows;
    every bucket set of comoments_cases with its time range dropped; every cell compared."""
    field = cc.main_table()[f]
    assert np.isfinite(field.values).all()
    groups, n_groups = (field.groups, 4) if grouped else (None, 1)
    for name, origin, width, n_buckets, _, _ in cc.bucket_sets(*_span(field)):
        for method, method_name in METHODS:
            got = hip.integral_buckets(field.batch, origin, width, n_buckets, groups=groups, method=method,
                                       n_groups=n_groups)
            expected = ic.oracle(field, groups, n_groups, origin, width, n_buckets, method)
            _, special = ic.assert_cells(got, expected, f"field {f} {name} {method_name} {n_groups} group(s)")
            assert special == 0


def test_a_link_that_crosses_many_buckets(hip):
    """Two one-point segments, (0, 1.0) and (10 000, 3.0): the only interval is the link between them. Width 100 at
    origin 0 (100 buckets) and at origin 50 (the first point lies before bucket 0, the second behind the last)."""
    field = cc.Field([_compress([0], [1.0]), _compress([10_000], [3.0])])
    assert len(field.batch) == 2 and field.ts.tolist() == [0, 10_000] and field.values.tolist() == [1.0, 3.0]
    for origin, n_buckets in ((0, 100), (50, 99)):
        starts = origin + 100 * np.arange(n_buckets)
        for method, name in METHODS:
            got = hip.integral_buckets(field.batch, origin, 100, n_buckets, method=method).reshape(n_buckets)
            ic.assert_cells(got.reshape(1, -1), ic.oracle(field, None, 1, origin, 100, n_buckets, method),
                            f"link {origin} {name}")
            assert (got["duration"] == 100).all()
            # the trapezoid under 1 + 2 t / 10 000 over [a, a + 100]: 100 + (2 a + 100) / 100, an exact f64; the kernel
            # rounds a handful of times (2^-53 each)
            exact = 100.0 * 1.0 if method == STEP else 100.0 + (2 * starts + 100) / 100.0
            assert np.allclose(got["integral"], exact, rtol=1e-13, atol=0.0)


def test_short_segments(hip):
    """Series 3 of the main table (runs of 2..12 points) alone, under every error bound: many short segments, every
    one linked to the next."""
    for f in (0, 1, 2):
        field = cc.Field([cc.main_table()[f].parts[3]])
        first, last = _span(field)
        assert len(field.ts) == 1500 and len(field.batch) >= 6
        for origin, width, n_buckets in ((first, last - first + 1, 1), (first, INTERVAL, (last - first) // INTERVAL + 1)):
            for method, name in METHODS:
                got = hip.integral_buckets(field.batch, origin, width, n_buckets, method=method)
                ic.assert_cells(got, ic.oracle(field, None, 1, origin, width, n_buckets, method), f"short {f} {width} {name}")
                assert int(got["duration"].sum()) == last - first
                if width == INTERVAL:
                    assert (got["duration"][0, :-1] == INTERVAL).all() and got["duration"][0, -1] == 0
    # segments of 1..5 points on irregular timestamps: as many links between segments as intervals inside them
    rng = np.random.default_rng(5)
    n = 600
    timestamps = 1_000 + np.cumsum(rng.integers(1, 400, n))
    values = datagen.sine_series(9, n)[1]
    cuts = np.concatenate([[0], np.minimum(np.cumsum(rng.integers(1, 6, n)), n)])
    cuts = cuts[:int(np.argmax(cuts == n)) + 1]
    tiny = cc.Field([_compress(timestamps[a:b], values[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(tiny.ts, timestamps) and len(tiny.batch) > n // 5
    first, last = _span(tiny)
    for origin, width, n_buckets in ((first - 55, 170, (last - first) // 170 + 2), (first, last - first, 1)):
        for method, name in METHODS:
            got = hip.integral_buckets(tiny.batch, origin, width, n_buckets, method=method)
            ic.assert_cells(got, ic.oracle(tiny, None, 1, origin, width, n_buckets, method), f"tiny {width} {name}")
            assert int(got["duration"].sum()) == last - first


def test_the_gap_rule(hip):
    field = cc.Field([cc.main_table()[0].parts[0]])   # regular, lossless
    first, last = _span(field)
    assert (np.diff(field.ts) == INTERVAL).all()
    args = (first - 30, 7 * INTERVAL, (last - first) // (7 * INTERVAL) + 2)
    for method, name in METHODS:
        below = hip.integral_buckets(field.batch, *args, method=method, max_gap=INTERVAL - 1)
        assert below.tobytes() == bytes(below.size * CELL.itemsize)
        ic.assert_cells(below, ic.oracle(field, None, 1, *args, method, INTERVAL - 1), f"gap below {name}")
        equal = hip.integral_buckets(field.batch, *args, method=method, max_gap=INTERVAL)
        ic.assert_cells(equal, ic.oracle(field, None, 1, *args, method, INTERVAL), f"gap equal {name}")
        assert int(equal["duration"].sum()) == last - first
        assert equal.tobytes() == hip.integral_buckets(field.batch, *args, method=method).tobytes()
    # holes of 10 and of 1 000 intervals, max_gap between them: exactly the long hole is lost
    n = 3_000
    steps = np.full(n - 1, INTERVAL, dtype=np.int64)
    steps[700], steps[1_900] = 10 * INTERVAL, 1_000 * INTERVAL
    timestamps = np.concatenate([[12_300], 12_300 + np.cumsum(steps)])
    holes = cc.Field([_compress(timestamps, datagen.sine_series(8, n)[1])])
    assert np.array_equal(holes.ts, timestamps)
    first, last = _span(holes)
    args = (first - 30, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2)
    for method, name in METHODS:
        for max_gap, lost in ((100 * INTERVAL, 1_000 * INTERVAL), (None, 0), (5 * INTERVAL, 1_010 * INTERVAL)):
            got = hip.integral_buckets(holes.batch, *args, method=method, max_gap=max_gap)
            ic.assert_cells(got, ic.oracle(holes, None, 1, *args, method, max_gap), f"holes {max_gap} {name}")
            assert int(got["duration"].sum()) == last - first - lost


def test_what_is_not_linked(hip):
    main = cc.main_table()[1]
    # a step back in time (the series boundaries of the main table) with groups=None: no link crosses them
    first, last = _span(main)
    series_time = sum(int(part_ts.max() - part_ts.min())
                      for part_ts in (main.ts[main.groups[main.segment] == k] for k in range(4)))
    for method, name in METHODS:
        got = hip.integral_buckets(main.batch, first, last - first + 1, 1, method=method)
        ic.assert_cells(got, ic.oracle(main, None, 1, first, last - first + 1, 1, method), f"boundaries {name}")
        assert int(got["duration"][0, 0]) == series_time
    # a group change in the middle of a series: the link between the two segments is lost, nothing else
    series = cc.Field([main.parts[0]])
    first, last = _span(series)
    cut = len(series.batch) // 2
    groups = (np.arange(len(series.batch)) >= cut).astype(np.uint32)
    rows_before = int(series.rows[:cut].sum())
    lost = int(series.ts[rows_before] - series.ts[rows_before - 1])
    assert lost > 0
    for method, name in METHODS:
        got = hip.integral_buckets(series.batch, first, 50 * INTERVAL, (last - first) // (50 * INTERVAL) + 1,
                                   groups=groups, method=method, n_groups=2)
        ic.assert_cells(got, ic.oracle(series, groups, 2, first, 50 * INTERVAL, (last - first) // (50 * INTERVAL) + 1,
                                       method), f"group change {name}")
        assert int(got["duration"].sum()) == last - first - lost
        assert int(got["duration"][0].sum()) == int(series.ts[rows_before - 1]) - first
    # equal timestamps: (500, 1) and (500, 2) are not linked; (500, 2) and (600, 4) are
    equal = cc.Field([_compress([500], [1.0]), _compress([500], [2.0]), _compress([600], [4.0])])
    assert equal.ts.tolist() == [500, 500, 600]
    for method, integral in ((LINEAR, 300.0), (STEP, 200.0)):
        got = hip.integral_buckets(equal.batch, 0, 1_000, 1, method=method)
        ic.assert_cells(got, ic.oracle(equal, None, 1, 0, 1_000, 1, method), "equal timestamps")
        assert got["duration"][0, 0] == 100 and got["integral"][0, 0] == integral


def test_constants(hip):
    """Levels held for 500 points each (PMC-Mean runs), buckets that divide the runs: in every cell that one level
    fills the average is within 2^-44 |c| of the level."""
    steps = cc.steps_table()[0]
    assert (steps.batch.model_type_id == mdb.MDB_PMC_MEAN_ID).all() and len(steps.batch) >= 12
    for intervals in (500, 250, 100):
        width, n_buckets = intervals * INTERVAL, 6000 // intervals
        for method, name in METHODS:
            got = hip.integral_buckets(steps.batch, 0, width, n_buckets, method=method)
            expected = ic.oracle(steps, None, 1, 0, width, n_buckets, method)
            ic.assert_cells(got, expected, f"constant {intervals} {name}")
            level = expected["level"]
            filled = ~np.isnan(level)
            assert filled.sum() >= n_buckets - 12
            average = mdb.integral_average(got)
            worst = np.abs(average[filled] - level[filled]) / np.abs(level[filled])
            print(f"constant {intervals} {name}: {int(filled.sum())} cells, |average - c| / |c| <= {worst.max():.3g} "
                  f"(allowed {ic.AVERAGE_TOLERANCE:.3g})")
            assert (np.abs(average[filled] - level[filled]) <= ic.AVERAGE_TOLERANCE * np.abs(level[filled])).all()
            if method == STEP:
                assert filled.all()   # (carried forward, the run's last interval holds its level too)


def test_step_is_interval_times_sum(hip):
    """A consistency check with an independent operator: on a regular series, STEP, origin at the first timestamp and
    width k * INTERVAL, every point of a bucket but the series' last carries INTERVAL microseconds: the integral is
    INTERVAL x agg_buckets' SUM."""
    for f in (0, 1):
        field = cc.Field([cc.main_table()[f].parts[0]])
        first, last = _span(field)
        assert (np.diff(field.ts) == INTERVAL).all()
        for k in (1, 9, 640):
            width, n_buckets = k * INTERVAL, (last - first) // (k * INTERVAL) + 1
            got = hip.integral_buckets(field.batch, first, width, n_buckets, method=STEP)
            expected = ic.oracle(field, None, 1, first, width, n_buckets, STEP)
            ic.assert_cells(got, expected, f"step {f} {k}")
            sums = hip.agg_buckets(field.batch, first, width, n_buckets, which_mask=mdb.MDB_AGG_SUM)["sum"]
            whole = np.arange(n_buckets) < (last - first) // width   # (not the bucket of the series' last point)
            assert whole.sum() >= n_buckets - 1
            error = np.abs(got["integral"][0, whole] - INTERVAL * sums[0, whole])
            assert (error <= ic.TOLERANCE * expected["scale"][0, whole]).all()


def test_rebucketing_and_origin_invariance(hip):
    field = cc.main_table()[2]
    first, last = _span(field)
    for width in (3 * INTERVAL, 3_333):
        origin, n_wide = first - 12_345, (last - first + 12_345) // (7 * width) + 2
        for method, name in METHODS:
            narrow = hip.integral_buckets(field.batch, origin, width, 7 * n_wide, groups=field.groups, method=method, n_groups=4)
            wide = hip.integral_buckets(field.batch, origin, 7 * width, n_wide, groups=field.groups, method=method, n_groups=4)
            expected = ic.oracle(field, field.groups, 4, origin, 7 * width, n_wide, method)
            ic.assert_cells(wide, expected, f"wide {width} {name}")
            np.testing.assert_array_equal(narrow["duration"].reshape(4, n_wide, 7).sum(axis=2), wide["duration"])
            folded = narrow["integral"].reshape(4, n_wide, 7).sum(axis=2)
            assert (np.abs(folded - wide["integral"]) <= ic.TOLERANCE * expected["scale"]).all()
            # the origin moved back by three widths with three more buckets: the cells that still exist, same bytes
            there = hip.integral_buckets(field.batch, origin - 3 * width, width, 7 * n_wide + 3, groups=field.groups,
                                         method=method, n_groups=4)
            assert np.ascontiguousarray(there[:, 3:]).tobytes() == narrow.tobytes()


@pytest.mark.parametrize("f", [0, 1], ids=["lossless", "abs5"])
def test_edge_table(hip, f):
    """NaN, +-0, +-inf, one- and two-point segments, epoch-scale Swing, width 2^40: each series a group. duration is
    exact everywhere; the integral is non-finite exactly where the reference says so."""
    field = cc.edge_table()[f]
    n_groups = len(field.parts)
    plain = special = 0
    for origin, width, n_buckets in ((0, 100, 40), (-35, 250, 24), (EDGE_EPOCH - 1000, 3000, 30),
                                     (EDGE_EPOCH, 50_000, 10), (0, 1 << 40, 3)):
        for method, name in METHODS:
            got = hip.integral_buckets(field.batch, origin, width, n_buckets, groups=field.groups, method=method,
                                       n_groups=n_groups)
            counts = ic.assert_cells(got, ic.oracle(field, field.groups, n_groups, origin, width, n_buckets, method),
                                     f"edge {origin} {width} {name}")
            plain, special = plain + counts[0], special + counts[1]
    assert plain > 0 and special > 0   # (both kinds of cell were among them)


def test_forms_and_runs_agree_and_cells_are_merged_into(hip, monkeypatch):
    field = cc.main_table()[1]
    batch, groups = field.batch, field.groups
    args = (-777, 1_300, 1_000)
    resident = field.resident(hip)
    cuts = [0, len(batch) // 5, len(batch) // 2, len(batch) - 7, len(batch)]   # (cuts inside series: links cross them)
    assert all(groups[c - 1] == groups[c] for c in cuts[1:-1])
    pairs = np.unique(field.segment * args[2] + (field.ts - args[0]) // args[1])   # (segment, bucket), oracle alone
    assert len(pairs) > 3 * 64
    for method, name in METHODS:
        expected = ic.oracle(field, groups, 4, *args, method)
        first = hip.integral_buckets(batch, *args, groups=groups, method=method, n_groups=4)
        ic.assert_cells(first, expected, f"host form {name}")
        assert hip.integral_buckets(batch, *args, groups=groups, method=method, n_groups=4).tobytes() == first.tobytes()
        assert hip.integral_buckets_list([batch], *args, groups=[groups], method=method, n_groups=4).tobytes() == first.tobytes()
        on_device = hip.integral_buckets_dev(resident, *args, groups=groups, method=method, n_groups=4)
        assert on_device.tobytes() == first.tobytes()
        assert hip.integral_buckets_dev(resident, *args, groups=groups, method=method, n_groups=4).tobytes() == first.tobytes()
        listed = hip.integral_buckets_list([batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])], *args,
                                           groups=[groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])], method=method,
                                           n_groups=4)
        assert listed.tobytes() == first.tobytes()
        # a second call merges into the cells of the first: both members doubled (x + x is exact)
        again = hip.integral_buckets(batch, *args, groups=groups, method=method, cells=first.copy())
        np.testing.assert_array_equal(again["duration"], 2 * first["duration"])
        np.testing.assert_array_equal(again["integral"], 2 * first["integral"])
        again = hip.integral_buckets_dev(resident, *args, groups=groups, method=method, cells=first.copy())
        np.testing.assert_array_equal(again["integral"], 2 * first["integral"])
        assert mdb.integral_merge(first.copy(), first).tobytes() == again.tobytes()
        # slices of 64 pairs, and the segments in another order (the sort path): rounding only
        order = np.random.default_rng(6).permutation(len(batch))
        monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "64")
        sliced = hip.integral_buckets(batch, *args, groups=groups, method=method, n_groups=4)
        sliced_one = hip.integral_buckets(batch, args[0], args[1] * args[2], 1, groups=groups, method=method, n_groups=4)
        monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
        ic.assert_cells(sliced, expected, f"slices of 64 pairs {name}")
        np.testing.assert_array_equal(sliced["duration"], first["duration"])
        ic.assert_cells(sliced_one, ic.oracle(field, groups, 4, args[0], args[1] * args[2], 1, method),
                        f"slices of 64 pairs, one bucket {name}")
        shuffled = cc.Field([batch.take(order)])
        moved = hip.integral_buckets(shuffled.batch, *args, groups=groups[order], method=method, n_groups=4)
        ic.assert_cells(moved, ic.oracle(shuffled, groups[order], 4, *args, method), f"shuffled {name}")


def test_the_convenience_is_one_bucket_over_the_span(hip):
    field = cc.main_table()[0]
    first, last = _span(field)
    cells = hip.integral(field.batch, groups=field.groups, n_groups=4, method=STEP, max_gap=INTERVAL)
    assert cells.shape == (4,)
    ic.assert_cells(cells.reshape(4, 1), ic.oracle(field, field.groups, 4, first, last - first + 1, 1, STEP, INTERVAL),
                    "integral()")
    assert hip.integral(field.batch.slice(0, 0), n_groups=2).tobytes() == bytes(2 * CELL.itemsize)


def test_errors_on_the_device_path_leave_the_cells_untouched(hip):
    field = cc.main_table()[1]
    batch, groups = field.parts[0], np.arange(len(field.parts[0]), dtype=np.uint32) % 3
    rng = np.random.default_rng(9)
    cells = np.frombuffer(rng.bytes(3 * 10 * CELL.itemsize), dtype=CELL).reshape(3, 10).copy()
    before = cells.copy()
    resident = hip.upload_segments(batch)
    # a group id out of range, on a row outside every bucket
    bad = groups.copy()
    bad[-1] = 3
    assert int(batch.start_time[-1]) > 10 * 1000 and int(batch.start_time[0]) < 10 * 1000
    for call in (lambda: hip.integral_buckets(batch, 0, 1000, 10, groups=bad, cells=cells, n_groups=3),
                 lambda: hip.integral_buckets_list([batch.slice(0, 5), batch.slice(5, len(batch))], 0, 1000, 10,
                                                   groups=[bad[:5], bad[5:]], cells=cells, n_groups=3),
                 lambda: hip.integral_buckets_dev(resident, 0, 1000, 10, groups=bad, cells=cells, n_groups=3)):
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
    for call in (lambda: hip.integral_buckets(broken, origin, width, 10, groups=groups, cells=cells),
                 lambda: hip.integral_buckets_dev(broken_resident, origin, width, 10, groups=groups, cells=cells)):
        with pytest.raises(mdb.HipError, match="model type"):
            call()
        assert cells.tobytes() == before.tobytes()
    broken_resident.free()
    # the request's own errors reach the device forms too, before `data` (a host pointer here) is touched
    request = hip._integral_request(0, 100, 10, 3, 7, None)
    data = cells.ctypes.data_as(ctypes.c_void_p)
    assert hip.lib.mdb_integral_buckets_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(request), data) == 1
    assert b"method" in hip.lib.mdb_last_error()
    assert cells.tobytes() == before.tobytes()
    # an empty batch and n_buckets == 0 succeed and change nothing
    hip.integral_buckets(batch.slice(0, 0), 0, 100, 10, cells=cells, n_groups=3)
    hip.integral_buckets_list([], 0, 100, 10, cells=cells, n_groups=3)
    assert cells.tobytes() == before.tobytes()
    none = np.zeros((3, 0), dtype=CELL)
    assert hip.integral_buckets(batch, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    assert hip.integral_buckets_dev(resident, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    resident.free()
