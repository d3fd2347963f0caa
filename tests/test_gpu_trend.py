"""The linear trend of a field over time on segments (mdb_trend_buckets*): per date_bin bucket and group one comoments
cell with x = the time offset of a point inside its bucket and y = its value. The tables are tests/comoments_cases.py's;
the reference (tests/trend_cases.py) takes the oracle's grid of a field, x = (t - origin) mod width from integers, and
each cell in exact arithmetic (math.fsum).

Tolerances are comoments_cases.assert_cells': count exact; each mean within 2^-44 of the cell's largest |x| or |v|; each
m2 within 1e-5 of its reference (so m2_x == 0.0 exactly in a cell of one timestamp); |c_xy - c_ref| <= 1e-5 *
sqrt(m2x_ref * m2y_ref). In a cell that holds a NaN or an infinity mean_y, m2_y and c_xy are not finite while mean_x
and m2_x are held to the reference all the same. Expected values never come from the library under test, except in the
tests that say they are consistency checks."""

import ctypes

import numpy as np
import pytest

import cases
import comoments_cases as cc
import datagen
import oracle_lib as ora
import trend_cases as tc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
CELL = mdb.COMOMENTS_CELL_DTYPE
EDGE_EPOCH = 1658671178037  # the first timestamp of the edge cases' epoch-scale series
# slope = c_xy / m2_x: the c_xy and m2_x tolerances and their product, rounded up
SLOPE_TOLERANCE = 3e-5


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()


def _span(field):
    return int(field.ts.min()), int(field.ts.max())


def _finish(cells, kind):
    return mdb.comoments_finish(cells, kind)


@pytest.mark.parametrize("f", [0, 1, 2], ids=["lossless", "rel1", "abs5"])
def test_parity_with_the_points_in_exact_arithmetic(hip, f):
    """All three model types, regular and irregular timestamps, segments far longer and far shorter than 64 rows."""
    field = cc.main_table()[f]
    for name, origin, width, n_buckets, t_lo, t_hi in cc.bucket_sets(*_span(field)):
        for groups, n_groups in ((field.groups, 4), (None, 1)):
            got = hip.trend_buckets(field.batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi,
                                    n_groups=n_groups)
            cc.assert_cells(got, tc.oracle(field, groups, n_groups, origin, width, n_buckets, t_lo, t_hi),
                            f"field {f} {name} {n_groups} group(s)")


@pytest.mark.parametrize("f", [0, 1], ids=["lossless", "abs5"])
def test_edge_table(hip, f):
    """NaN, +-0, +-inf, one- and two-point segments, epoch-scale Swing, width 2^40: each series a group. count is
    agg_buckets'; the x side stays finite and right where a value is not."""
    field = cc.edge_table()[f]
    n_groups = len(field.parts)
    special = 0
    for origin, width, n_buckets, t_lo, t_hi in ((0, 100, 40, I64_MIN, I64_MAX), (-35, 250, 24, 150, 950),
                                                 (EDGE_EPOCH - 1000, 3000, 30, I64_MIN, I64_MAX),
                                                 (EDGE_EPOCH, 50_000, 10, EDGE_EPOCH + 100_500, EDGE_EPOCH + 300_400),
                                                 (0, 1 << 40, 3, I64_MIN, I64_MAX)):
        got = hip.trend_buckets(field.batch, origin, width, n_buckets, groups=field.groups, t_lo=t_lo, t_hi=t_hi,
                                n_groups=n_groups)
        expected = tc.oracle(field, field.groups, n_groups, origin, width, n_buckets, t_lo, t_hi)
        cc.assert_cells(got, expected, f"edge {origin} {width}")
        special += tc.assert_x_side(got, expected, f"edge {origin} {width}")
        np.testing.assert_array_equal(got["count"], hip.agg_buckets(field.batch, origin, width, n_buckets,
                                                                    groups=field.groups, t_lo=t_lo, t_hi=t_hi,
                                                                    n_groups=n_groups)["count"])
    assert special > 0   # (cells with a NaN or an infinity were among them)


def test_a_constant_field_has_no_trend(hip):
    """Long PMC-Mean runs, buckets that divide the runs: c_xy, m2_y and the slope are 0.0 exactly, corr is NaN, and
    m2_x is the closed form delta^2 * n(n^2-1)/12 against Python integers."""
    steps = cc.steps_table()[0]
    assert (steps.batch.model_type_id == mdb.MDB_PMC_MEAN_ID).all() and len(steps.batch) >= 12
    for intervals in (500, 250, 100):
        width, n_buckets = intervals * INTERVAL, 6000 // intervals
        got = hip.trend_buckets(steps.batch, 0, width, n_buckets)
        cc.assert_cells(got, tc.oracle(steps, None, 1, 0, width, n_buckets), f"constant {intervals}")
        assert (got["count"] == intervals).all()
        assert (got["c_xy"] == 0.0).all() and (got["m2_y"] == 0.0).all()
        assert (_finish(got, "regr_slope") == 0.0).all()
        assert np.isnan(_finish(got, "corr")).all()
        n = intervals
        exact = INTERVAL * INTERVAL * n * (n * n - 1) / 12   # (an integer: three consecutive numbers, times 100^2)
        assert INTERVAL * INTERVAL * n * (n * n - 1) % 12 == 0
        assert (np.abs(got["m2_x"] - exact) <= cc.M2_TOLERANCE * exact).all()
        assert (np.abs(got["mean_x"] - INTERVAL * (n - 1) / 2) <= cc.MEAN_TOLERANCE * INTERVAL * (n - 1)).all()


def test_an_exact_ramp(hip):
    """v = 100 + k on regular timestamps, lossless: Swing segments, slope 1 / INTERVAL, r2 1 and the intercept the
    bucket's first value."""
    n = 3_000
    timestamps = np.arange(n, dtype=np.int64) * INTERVAL
    values = (100.0 + np.arange(n)).astype(np.float32)
    batch = ora.try_compress_univariate_time_series(timestamps, values, cases.LOSSLESS)
    assert (batch.model_type_id == mdb.MDB_SWING_ID).any()
    rebuilt = ora.grid_batch(batch)[1]
    assert np.array_equal(rebuilt.astype(np.float32), values)
    slope_ref = 1.0 / INTERVAL
    for intervals in (64, 700, 3_000):
        width, n_buckets = intervals * INTERVAL, -(-n // intervals)
        got = hip.trend_buckets(batch, 0, width, n_buckets).reshape(n_buckets)
        slope, r2 = _finish(got, "regr_slope"), _finish(got, "regr_r2")
        intercept = _finish(got, "regr_intercept")
        first_value = 100.0 + np.arange(n_buckets) * intervals
        print(f"ramp {intervals}: slope error {np.abs(slope / slope_ref - 1).max():.3g}, r2 error "
              f"{np.abs(r2 - 1).max():.3g}, intercept error {np.abs(intercept - first_value).max():.3g}")
        assert (got["count"] >= 2).all()
        assert (np.abs(slope - slope_ref) <= SLOPE_TOLERANCE * slope_ref).all()
        assert (np.abs(r2 - 1.0) <= SLOPE_TOLERANCE).all()
        # mean_y and slope * mean_x within the mean tolerance, and the slope's error over at most one width
        allowed = cc.MEAN_TOLERANCE * (100.0 + n + slope_ref * width) + SLOPE_TOLERANCE * slope_ref * width
        assert (np.abs(intercept - first_value) <= allowed).all()


def test_one_point_and_one_timestamp(hip):
    """Buckets of one interval hold one point: m2_x == 0.0 and no slope. Two series of one group that share every
    timestamp: count 2, m2_x == 0.0 still, no slope."""
    steps, noisy = cc.steps_table()
    got = hip.trend_buckets(noisy.batch, 0, INTERVAL, 6000)
    cc.assert_cells(got, tc.oracle(noisy, None, 1, 0, INTERVAL, 6000), "one point a cell")
    assert (got["count"] == 1).all() and (got["m2_x"] == 0.0).all() and (got["mean_x"] == 0.0).all()
    assert np.isnan(_finish(got, "regr_slope")).all() and np.isnan(_finish(got, "corr")).all()
    both = mdb.SegmentBatch.concat([steps.batch, noisy.batch])
    got = hip.trend_buckets(both, -30, INTERVAL, 6001)
    assert (got["count"][0, :6000] == 2).all() and got["count"][0, 6000] == 0
    assert (got["m2_x"] == 0.0).all() and (got["mean_x"][0, :6000] == 30.0).all()
    assert (got["m2_y"][0, :6000] > 0.0).any() and (got["c_xy"] == 0.0).all()
    for kind in ("regr_slope", "regr_intercept", "regr_r2", "corr"):
        assert np.isnan(_finish(got, kind)).all()


def test_the_y_side_is_moments_buckets(hip):
    """A consistency check: comoments_moments(cells, "y") against moments_buckets of the same call, both held to the
    reference with the moments' tolerance."""
    field = cc.main_table()[1]
    first, last = _span(field)
    args = (first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2)
    cells = hip.trend_buckets(field.batch, *args, groups=field.groups, n_groups=4)
    y_side = mdb.comoments_moments(cells, "y")
    moments = hip.moments_buckets(field.batch, *args, groups=field.groups, n_groups=4)
    expected = tc.oracle(field, field.groups, 4, *args)
    np.testing.assert_array_equal(y_side["count"], moments["count"])
    hit = moments["count"] > 0
    for got in (y_side, moments):
        assert (np.abs(got["mean"][hit] - expected["mean_y"][hit]) <= cc.MEAN_TOLERANCE * expected["largest_y"][hit]).all()
        assert (np.abs(got["m2"][hit] - expected["m2_y"][hit]) <= cc.M2_TOLERANCE * expected["m2_y"][hit]).all()


def test_forms_and_runs_agree_bit_for_bit(hip):
    field = cc.main_table()[1]
    batch, groups = field.batch, field.groups
    args = (-777, 1_300, 1_000)
    first = hip.trend_buckets(batch, *args, groups=groups, n_groups=4)
    expected = tc.oracle(field, groups, 4, *args)
    cc.assert_cells(first, expected, "host form")
    assert hip.trend_buckets(batch, *args, groups=groups, n_groups=4).tobytes() == first.tobytes()
    assert hip.trend_buckets_list([batch], *args, groups=[groups], n_groups=4).tobytes() == first.tobytes()
    resident = field.resident(hip)
    on_device = hip.trend_buckets_dev(resident, *args, groups=groups, n_groups=4)
    assert on_device.tobytes() == first.tobytes()
    assert hip.trend_buckets_dev(resident, *args, groups=groups, n_groups=4).tobytes() == first.tobytes()
    cuts = [0, len(batch) // 5, len(batch) // 2, len(batch) - 7, len(batch)]   # (the batch cut at three places)
    listed = hip.trend_buckets_list([batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])], *args,
                                    groups=[groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])], n_groups=4)
    cc.assert_cells(listed, expected, "list form, three cuts")


def test_small_slices_and_permuted_segments(hip, monkeypatch):
    """Several slices, two levels of the reduction tree and the sort path: each held to the reference."""
    field = cc.main_table()[1]
    batch, groups = field.batch, field.groups
    first, last = _span(field)
    args = (first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2)
    wide = (first, last - first + 1, 1)     # (every pair of a series in one cell: runs through the tree)
    order = np.random.default_rng(6).permutation(len(batch))
    shuffled = cc.Field([batch.take(order)])
    slice_pairs = 300                       # (more than one 64-entry tile: two levels)
    pairs = np.unique(field.segment * args[2] + (field.ts - args[0]) // args[1])   # (segment, bucket), oracle alone
    assert len(pairs) > 3 * slice_pairs and len(batch) > 64
    monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", str(slice_pairs))
    sliced = hip.trend_buckets(batch, *args, groups=groups, n_groups=4)
    sliced_wide = hip.trend_buckets(batch, *wide, groups=groups, n_groups=4)
    sliced_shuffled = hip.trend_buckets(shuffled.batch, *args, groups=groups[order], n_groups=4)
    sliced_shuffled_wide = hip.trend_buckets(shuffled.batch, *wide, groups=groups[order], n_groups=4)
    monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
    cc.assert_cells(sliced, tc.oracle(field, groups, 4, *args), "slices of 300 pairs")
    cc.assert_cells(sliced_wide, tc.oracle(field, groups, 4, *wide), "slices of 300 pairs, one bucket")
    cc.assert_cells(sliced_shuffled, tc.oracle(shuffled, groups[order], 4, *args), "slices, shuffled")
    cc.assert_cells(sliced_shuffled_wide, tc.oracle(shuffled, groups[order], 4, *wide), "slices, shuffled, one bucket")
    whole = hip.trend_buckets(shuffled.batch, *args, groups=groups[order], n_groups=4)
    cc.assert_cells(whole, tc.oracle(shuffled, groups[order], 4, *args), "shuffled (sort path)")


def test_two_calls_accumulate(hip):
    field = cc.main_table()[2]
    batch, groups = field.batch, field.groups
    first, last = _span(field)
    args = (first - 40, 170 * INTERVAL, (last - first) // (170 * INTERVAL) + 2)
    expected = tc.oracle(field, groups, 4, *args)
    half = len(batch) // 2
    cells = hip.trend_buckets(batch.slice(0, half), *args, groups=groups[:half], n_groups=4)
    separately = hip.trend_buckets(batch.slice(half, len(batch)), *args, groups=groups[half:], n_groups=4)
    merged = mdb.comoments_merge(cells.copy(), separately)
    cells = hip.trend_buckets(batch.slice(half, len(batch)), *args, groups=groups[half:], cells=cells)
    cc.assert_cells(cells, expected, "two calls into the same cells")
    cc.assert_cells(merged, expected, "comoments_merge of two fresh results")


def test_origin_invariance(hip):
    """The origin moved back by three widths with three more buckets: the cells that still exist have the same bytes."""
    field = cc.main_table()[0]
    first, last = _span(field)
    for width in (7 * INTERVAL, 3_333):
        origin, n_buckets = first - 12_345, (last - first + 12_345) // width + 2
        here = hip.trend_buckets(field.batch, origin, width, n_buckets, groups=field.groups, n_groups=4)
        there = hip.trend_buckets(field.batch, origin - 3 * width, width, n_buckets + 3, groups=field.groups, n_groups=4)
        assert (there["count"][:, :3] == 0).all() and int(here["count"].sum()) == len(field.ts)
        assert np.ascontiguousarray(there[:, 3:]).tobytes() == here.tobytes()


def test_macaque_v_through_the_cursor_index_and_without(hip, monkeypatch):
    """Lossless MacaqueV streams of 65 536 values, regular and irregular timestamps: piece by piece from the cursor
    index (k_trend_pieces) with buckets that cut the pieces of 64 values in the middle, and one lane per stream with
    MDB_GRID_MV_INDEX=0."""
    n = 140_000
    rng = np.random.default_rng(43)
    regular = np.arange(n, dtype=np.int64) * INTERVAL
    irregular = np.concatenate([[0], np.cumsum(rng.integers(50, 150, n - 1))]).astype(np.int64)
    parts = []
    for k, timestamps in enumerate((regular, irregular)):
        values = datagen.sine_series(21 + k, n)[1]
        offsets = np.append(np.arange(0, n, 65536), n).astype(np.uint64)
        parts.append(hip.compress_chunks(timestamps, values, offsets, cases.LOSSLESS))
    field = cc.Field(parts)
    batch, groups = field.batch, field.groups
    assert int((batch.model_type_id == mdb.MDB_MACAQUE_V_ID).sum()) >= 4
    resident = field.resident(hip)
    try:
        for origin, width, n_buckets in ((0, 777 * INTERVAL, 190), (13, 41 * INTERVAL + 7, 3_500)):
            expected = tc.oracle(field, groups, 2, origin, width, n_buckets)
            hip.profile_enable(True)
            hip.profile_reset()
            got = hip.trend_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=2)
            kernels = hip.profile()
            assert "k_trend_pieces" in kernels and "k_trend_partials" in kernels, sorted(kernels)
            cc.assert_cells(got, expected, f"index {width}")
            on_device = hip.trend_buckets_dev(resident, origin, width, n_buckets, groups=groups, n_groups=2)
            assert on_device.tobytes() == got.tobytes()
            monkeypatch.setenv("MDB_GRID_MV_INDEX", "0")
            hip.profile_reset()
            serial = hip.trend_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=2)
            kernels = hip.profile()
            monkeypatch.delenv("MDB_GRID_MV_INDEX")
            assert "k_trend_pieces" not in kernels and "k_trend_partials" in kernels, sorted(kernels)
            cc.assert_cells(serial, expected, f"no index {width}")
    finally:
        hip.profile_enable(False)
        field.free()


def test_the_convenience_returns_its_origin(hip):
    """Context.trend: one bucket over the data inside the range, x counted from the returned origin."""
    field = cc.main_table()[1]
    first, last = _span(field)
    t_lo, t_hi = first + 7_777, last - 12_321
    cells, origin = hip.trend(field.batch, t_lo, t_hi, groups=field.groups, n_groups=4)
    assert origin == t_lo and cells.shape == (4,)
    expected = tc.oracle(field, field.groups, 4, origin, t_hi - origin + 1, 1, t_lo, t_hi)
    cc.assert_cells(cells.reshape(4, 1), expected, "trend()")
    cells, origin = hip.trend(field.batch, t_lo, t_hi, groups=field.groups, n_groups=4, origin=first - 5)
    assert origin == first - 5
    cc.assert_cells(cells.reshape(4, 1), tc.oracle(field, field.groups, 4, origin, t_hi - origin + 1, 1, t_lo, t_hi),
                    "trend(origin=)")
    cells, _ = hip.trend(field.batch, last + 10, last + 1000, groups=field.groups, n_groups=4)
    assert cells.tobytes() == bytes(4 * CELL.itemsize)


def test_errors_leave_the_cells_untouched(hip):
    field = cc.main_table()[1]
    batch, groups = field.parts[0], np.arange(len(field.parts[0]), dtype=np.uint32) % 3
    rng = np.random.default_rng(9)
    cells = np.frombuffer(rng.bytes(3 * 10 * CELL.itemsize), dtype=CELL).reshape(3, 10).copy()
    before = cells.copy()
    resident = hip.upload_segments(batch)
    seg = batch.as_c()
    group_pointer = groups.ctypes.data_as(ctypes.c_void_p)
    data = cells.ctypes.data_as(ctypes.c_void_p)
    for origin, width, n_groups, which_mask, message in ((0, 100, 3, 1, b"which_mask"), (0, 0, 3, 0, b"width"),
                                                         (0, -5, 3, 0, b"width"), (0, 100, 0, 0, b"n_groups")):
        request = _abi.BucketRequestC(origin, width, 10, I64_MIN, I64_MAX, n_groups, which_mask)
        pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
        group_pointers = (ctypes.c_void_p * 1)(group_pointer.value)
        assert hip.lib.mdb_trend_buckets(hip.handle, ctypes.byref(seg), group_pointer, ctypes.byref(request), data) == 1
        assert message in hip.lib.mdb_last_error()
        assert hip.lib.mdb_trend_buckets_list(hip.handle, pointers, group_pointers, 1, ctypes.byref(request), data) == 1
        assert message in hip.lib.mdb_last_error()
        # (fails before `data`, a host pointer here, is touched)
        assert hip.lib.mdb_trend_buckets_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(request), data) == 1
        assert message in hip.lib.mdb_last_error()
        assert cells.tobytes() == before.tobytes()
    # a group id out of range, on a row the time range leaves out
    bad = groups.copy()
    bad[-1] = 3
    t_hi = int(batch.start_time[len(batch) // 2])
    assert int(batch.start_time[-1]) > t_hi
    for call in (lambda: hip.trend_buckets(batch, 0, 1000, 10, groups=bad, t_hi=t_hi, cells=cells),
                 lambda: hip.trend_buckets_list([batch.slice(0, 5), batch.slice(5, len(batch))], 0, 1000, 10,
                                                groups=[bad[:5], bad[5:]], t_hi=t_hi, cells=cells),
                 lambda: hip.trend_buckets_dev(resident, 0, 1000, 10, groups=bad, t_hi=t_hi, cells=cells)):
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
    for call in (lambda: hip.trend_buckets(broken, origin, width, 10, groups=groups, cells=cells),
                 lambda: hip.trend_buckets_dev(broken_resident, origin, width, 10, groups=groups, cells=cells)):
        with pytest.raises(mdb.HipError, match="model type"):
            call()
        assert cells.tobytes() == before.tobytes()
    broken_resident.free()
    # NULL arguments
    request = _abi.BucketRequestC(0, 100, 10, I64_MIN, I64_MAX, 3, 0)
    assert hip.lib.mdb_trend_buckets(hip.handle, None, None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_trend_buckets(hip.handle, ctypes.byref(seg), None, None, data) == 1
    assert hip.lib.mdb_trend_buckets(hip.handle, ctypes.byref(seg), None, ctypes.byref(request), None) == 1
    assert hip.lib.mdb_trend_buckets(None, ctypes.byref(seg), None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_trend_buckets_dev(hip.handle, None, None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_trend_buckets_list(hip.handle, None, None, 1, ctypes.byref(request), data) == 1
    assert b"NULL" in hip.lib.mdb_last_error()
    assert cells.tobytes() == before.tobytes()
    # an empty batch and n_buckets == 0 succeed and change nothing
    hip.trend_buckets(batch.slice(0, 0), 0, 100, 10, cells=cells, n_groups=3)
    hip.trend_buckets_list([], 0, 100, 10, cells=cells, n_groups=3)
    assert cells.tobytes() == before.tobytes()
    none = np.zeros((3, 0), dtype=CELL)
    assert hip.trend_buckets(batch, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    assert hip.trend_buckets_dev(resident, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    resident.free()
