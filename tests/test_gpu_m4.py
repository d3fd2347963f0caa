"""M4 downsampling on segments (mdb_m4_buckets*): per date_bin bucket and group the first, last, lowest and highest
point with their timestamps, and the count. The oracle is ora.grid_batch's points reduced per cell in numpy by the
four rules - a lexsort per rule on (t, key) with key the totalOrder key of the f32 bits. Timestamps, the bit patterns
of the values and the counts must be exact: no test has a tolerance."""

import ctypes

import numpy as np
import pytest

import cases
import layouts
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

INTERVAL = 100  # the sampling interval of tests/datagen.py
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ALL = mdb.MDB_AGG_COUNT | mdb.MDB_AGG_MIN | mdb.MDB_AGG_MAX | mdb.MDB_AGG_SUM


from m4_cases import (GRIDS as _GRIDS, POINTS, keys_of as _keys, point_buckets as _point_buckets, reduce as _reduce,
                      grid as _grid, oracle as _oracle, assert_cells as _assert_cells)


def _series_batch(eb, irregular, n_series=3, length=6000, seed=400):
    parts = [cases.mixed_batch(eb, irregular, seed=seed + k, length=length)[2] for k in range(n_series)]
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    return mdb.SegmentBatch.concat(parts), groups


def _bucket_sets(first, last):
    """(name, origin, width, n_buckets, t_lo, t_hi) over data in [first, last]: those of test_gpu_agg_buckets."""
    span = last - first + 1
    return [
        ("width_1_interval", first, INTERVAL, span // INTERVAL + 1, I64_MIN, I64_MAX),
        ("width_7_intervals", first, 7 * INTERVAL, span // (7 * INTERVAL) + 1, I64_MIN, I64_MAX),
        ("width_1000_intervals", first, 1000 * INTERVAL, span // (1000 * INTERVAL) + 1, I64_MIN, I64_MAX),
        ("one_bucket", first, span, 1, I64_MIN, I64_MAX),
        ("unaligned_origin_before", first - 12_345, 3_333, (span + 12_345) // 3_333 + 2, I64_MIN, I64_MAX),
        ("buckets_after_the_data", last + 1, 1000, 50, I64_MIN, I64_MAX),
        ("range_cuts_buckets", first - 50, 5_000, span // 5_000 + 2, first + 7_777, last - 12_321),
    ]


@pytest.mark.parametrize("eb_name", ["lossless", "rel5", "abs5"])
@pytest.mark.parametrize("irregular", [False, True], ids=["regular", "irregular"])
def test_parity_with_the_points_reduced_by_the_four_rules(hip, eb_name, irregular):
    batch, groups = _series_batch(cases.error_bounds()[eb_name], irregular)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    for name, origin, width, n_buckets, t_lo, t_hi in _bucket_sets(first, last):
        got = hip.m4_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
        _assert_cells(got, _oracle(batch, groups, 3, origin, width, n_buckets, t_lo, t_hi), f"{eb_name} {name}")


@pytest.mark.parametrize("eb_name", ["lossless", "rel5"])
def test_edge_case_series(hip, eb_name):
    """NaN, infinities, one- and two-point segments, long residual tails, huge timestamp gaps: each series a group."""
    eb = cases.error_bounds()[eb_name]
    parts = [ora.try_compress_univariate_time_series(ts, v, eb) for _, ts, v in cases.edge_case_series()]
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    batch = mdb.SegmentBatch.concat(parts)
    for origin, width, n_buckets in ((0, 100, 40), (-35, 250, 24), (1658671178037 - 1000, 3000, 30), (0, 1 << 40, 3)):
        got = hip.m4_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=len(parts))
        _assert_cells(got, _oracle(batch, groups, len(parts), origin, width, n_buckets), f"{eb_name} {origin} {width}")


@pytest.mark.parametrize("direction", ["rising", "falling"])
def test_swing_ties_report_the_earliest_point_of_the_run(hip, direction):
    """Ramps whose step is about a sixth of an f32 ulp of their level: consecutive points of a Swing segment round to
    the same f32, and the far extreme of a bucket is the EARLIEST point of its last run, not the bucket's last point."""
    n = 2000
    timestamps = 1_700_000_000_000_000 + np.arange(n, dtype=np.int64) * INTERVAL
    ramp = np.arange(n, dtype=np.float64) * 1e-5
    values = (1000.0 + (ramp if direction == "rising" else -ramp)).astype(np.float32)
    batch = ora.try_compress_univariate_time_series(timestamps, values, mdb.error_bound("absolute", 0.002))
    lengths = _grid(batch)[2]
    swing = batch.model_type_id == mdb.MDB_SWING_ID
    assert swing.any() and int(lengths[swing].max()) >= 64
    grid_values = _grid(batch)[1]
    assert int((np.diff(grid_values) == 0).sum()) > n // 2   # runs of equal values in what is reduced
    first = int(timestamps[0])
    far_is_late = 0
    for points in (7, 64):
        width, n_buckets = points * INTERVAL, n // points + 1
        got = hip.m4_buckets(batch, first - 3 * INTERVAL, width, n_buckets + 1)
        expected = _oracle(batch, None, 1, first - 3 * INTERVAL, width, n_buckets + 1)
        _assert_cells(got, expected, f"{direction} {points}")
        full = expected["count"] == points
        far = expected["t_max" if direction == "rising" else "t_min"]
        far_is_late += int((far[full] < expected["t_last"][full]).sum())
    assert far_is_late > 0   # (the oracle's far extreme does sit in front of the last point somewhere)


def test_equal_timestamps_in_one_group_and_the_sort_path(hip):
    """Two different series with the same timestamps in one group: first / last follow (t, key). The same rows
    shuffled go through the sort path and give identical bytes."""
    parts = [cases.mixed_batch(cases.error_bounds()["rel5"], False, seed=460 + k, length=6000)[2] for k in range(2)]
    batch = mdb.SegmentBatch.concat(parts)
    assert int(parts[0].start_time.min()) == int(parts[1].start_time.min())
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    args = (first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2)
    got = hip.m4_buckets(batch, *args)
    expected = _oracle(batch, None, 1, *args)
    _assert_cells(got, expected, "two series, one group")
    assert (expected["v_first"].view(np.uint32) != expected["v_last"].view(np.uint32)).any()
    shuffled = batch.take(np.random.default_rng(6).permutation(len(batch)))
    assert hip.m4_buckets(shuffled, *args).tobytes() == got.tobytes()
    one_point = hip.m4_buckets(batch, first, INTERVAL, 50)   # (both series' point in every bucket: ties on t)
    _assert_cells(one_point, _oracle(batch, None, 1, first, INTERVAL, 50), "one timestamp per bucket")
    assert (one_point["count"] == 2).all() and (one_point["t_first"] == one_point["t_last"]).all()


def test_runs_of_one_cell_through_every_level_of_the_reduction_tree(hip):
    """More than 4 096 pairs in one cell: level 0's tiles, then levels 1 and 2 - in pair order (one bucket) and on the
    sort path (two buckets over copies of one series)."""
    base, _ = _series_batch(cases.error_bounds()["rel5"], False, n_series=1, length=6000, seed=440)
    big = base.take(np.tile(np.arange(len(base)), 5000 // len(base) + 2))
    assert len(big) > 4096
    first, last = int(big.start_time.min()), int(big.end_time.max())
    resident = hip.upload_segments(big)
    for width, n_buckets in ((last - first + 1, 1), ((last - first) // 2 + 1, 2)):
        got = hip.m4_buckets(big, first, width, n_buckets)
        _assert_cells(got, _oracle(big, None, 1, first, width, n_buckets), f"{n_buckets} bucket(s)")
        assert hip.m4_buckets_dev(resident, first, width, n_buckets).tobytes() == got.tobytes()
    resident.free()


def test_macaque_v_through_the_cursor_index_and_without(hip, monkeypatch):
    """Lossless MacaqueV streams of 65 536 values, regular and irregular timestamps: piece by piece from the cursor
    index (k_m4_pieces), and one lane per stream with MDB_GRID_MV_INDEX=0."""
    import datagen
    n = 140_000
    rng = np.random.default_rng(43)
    regular = np.arange(n, dtype=np.int64) * INTERVAL
    irregular = np.concatenate([[0], np.cumsum(rng.integers(50, 150, n - 1))]).astype(np.int64)
    parts = []
    for k, timestamps in enumerate((regular, irregular)):
        values = datagen.sine_series(21 + k, n)[1]
        offsets = np.append(np.arange(0, n, 65536), n).astype(np.uint64)
        parts.append(hip.compress_chunks(timestamps, values, offsets, cases.LOSSLESS))
    batch = mdb.SegmentBatch.concat(parts)
    assert int((batch.model_type_id == mdb.MDB_MACAQUE_V_ID).sum()) >= 4
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    resident = hip.upload_segments(batch)
    try:
        for origin, width, n_buckets in ((0, 777 * INTERVAL, 190), (13, 3 * INTERVAL, 48_000)):
            expected = _oracle(batch, groups, 2, origin, width, n_buckets)
            hip.profile_enable(True)
            hip.profile_reset()
            got = hip.m4_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=2)
            kernels = hip.profile()
            assert "k_m4_pieces" in kernels and "k_m4_partials" in kernels, sorted(kernels)
            _assert_cells(got, expected, f"index {width}")
            assert hip.m4_buckets_dev(resident, origin, width, n_buckets, groups=groups, n_groups=2).tobytes() == got.tobytes()
            monkeypatch.setenv("MDB_GRID_MV_INDEX", "0")
            hip.profile_reset()
            serial = hip.m4_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=2)
            kernels = hip.profile()
            monkeypatch.delenv("MDB_GRID_MV_INDEX")
            assert "k_m4_pieces" not in kernels and "k_m4_partials" in kernels, sorted(kernels)
            _assert_cells(serial, expected, f"no index {width}")
    finally:
        hip.profile_enable(False)
        resident.free()


def test_determinism_across_runs_forms_slices_and_halves(hip, monkeypatch):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, n_series=4, length=20_000, seed=420)
    lossless, lossless_groups = _series_batch(cases.LOSSLESS, True, n_series=2, length=8_000, seed=430)
    batch = mdb.SegmentBatch.concat([batch, lossless])
    groups = np.concatenate([groups, lossless_groups + 4])
    args = (-777, 1_300, 1_600)
    first = hip.m4_buckets(batch, *args, groups=groups, n_groups=6)
    _assert_cells(first, _oracle(batch, groups, 6, *args), "default")
    assert hip.m4_buckets(batch, *args, groups=groups, n_groups=6).tobytes() == first.tobytes()
    cut = [0, len(batch) // 3, 2 * len(batch) // 3, len(batch)]
    listed = hip.m4_buckets_list([batch.slice(cut[k], cut[k + 1]) for k in range(3)], *args,
                                 groups=[groups[cut[k]:cut[k + 1]] for k in range(3)], n_groups=6)
    assert listed.tobytes() == first.tobytes()
    resident = hip.upload_segments(batch)
    assert hip.m4_buckets_dev(resident, *args, groups=groups, n_groups=6).tobytes() == first.tobytes()
    resident.free()
    monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "1000")
    sliced = hip.m4_buckets(batch, *args, groups=groups, n_groups=6)
    monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
    assert sliced.tobytes() == first.tobytes()   # (bytes: unlike SUM, nothing here depends on an order)
    half = len(batch) // 2
    folded = hip.m4_buckets(batch.slice(half, len(batch)), *args, groups=groups[half:], n_groups=6)
    second_half = folded.copy()
    folded = hip.m4_buckets(batch.slice(0, half), *args, groups=groups[:half], cells=folded)
    assert folded.tobytes() == first.tobytes()
    first_half = hip.m4_buckets(batch.slice(0, half), *args, groups=groups[:half], n_groups=6)
    assert mdb.m4_merge(first_half, second_half).tobytes() == first.tobytes()
    one_group = hip.m4_buckets(batch, *args)   # (keys out of order across series: the sort path)
    _assert_cells(one_group, _oracle(batch, None, 1, *args), "one group")


def test_relation_to_agg_buckets(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    for _, origin, width, n_buckets, t_lo, t_hi in _bucket_sets(first, last)[1:]:
        cells = hip.m4_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
        states = hip.agg_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
        np.testing.assert_array_equal(cells["count"], states["count"])
        hit = cells["count"] > 0
        assert not np.isnan(cells["v_min"][hit]).any() and not np.isnan(cells["v_max"][hit]).any()
        assert (cells["v_min"][hit] == states["min"][hit]).all() and (cells["v_max"][hit] == states["max"][hit]).all()


def test_cells_that_receive_nothing_keep_their_bytes(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, length=2000)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    origin, width, n_buckets = first - 10 * 3_000, 3_000, (last - first) // 3_000 + 30
    expected = _oracle(batch, groups, 4, origin, width, n_buckets)   # (group 3 has no segment)
    empty = expected["count"] == 0
    assert empty[:3].any() and empty[3].all() and (~empty).any()
    cells = mdb.fresh_m4_cells((4, n_buckets))
    cells.view(np.uint8).reshape(4, n_buckets, -1)[empty] = 0xA5
    pattern = cells.copy()
    for form in ("host", "dev"):
        got = cells.copy()
        if form == "host":
            hip.m4_buckets(batch, origin, width, n_buckets, groups=groups, cells=got)
        else:
            resident = hip.upload_segments(batch)
            hip.m4_buckets_dev(resident, origin, width, n_buckets, groups=groups, cells=got)
            resident.free()
        assert got[empty].tobytes() == pattern[empty].tobytes(), form
        _assert_cells(got[~empty], expected[~empty], form)


def test_negative_timestamps_floor(hip):
    timestamps = np.arange(-5000, 5000, 100, dtype=np.int64)
    values = (np.sin(np.arange(len(timestamps)) / 7.0) * 50).astype(np.float32)
    for eb in (cases.LOSSLESS, mdb.error_bound("absolute", 5.0)):
        batch = ora.try_compress_univariate_time_series(timestamps, values, eb)
        for origin, width, n_buckets in ((-4950, 300, 40), (-10_000, 1_000, 20), (7, 450, 30), (-3001, 1, 2500)):
            got = hip.m4_buckets(batch, origin, width, n_buckets)
            _assert_cells(got, _oracle(batch, None, 1, origin, width, n_buckets), f"{origin} {width}")


def test_extreme_origin_and_width_do_not_overflow(hip):
    timestamps = np.array([-(1 << 62), -5, 0, 17, 1 << 40, (1 << 62) + 3], dtype=np.int64)
    values = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], dtype=np.float32)
    batch = ora.try_compress_univariate_time_series(timestamps, values, cases.LOSSLESS)
    for origin, width, n_buckets, t_lo, t_hi in ((I64_MIN, (1 << 62) - 1, 8, I64_MIN, I64_MAX),
                                                 (I64_MIN + 1, 1 << 62, 4, I64_MIN, I64_MAX),
                                                 (I64_MIN, I64_MAX, 2, I64_MIN, I64_MAX),
                                                 (I64_MAX - 10, 1 << 62, 3, I64_MIN, I64_MAX),
                                                 (-(1 << 62), 1 << 61, 5, -100, I64_MAX)):
        got = hip.m4_buckets(batch, origin, width, n_buckets, t_lo=t_lo, t_hi=t_hi)
        _assert_cells(got, _oracle(batch, None, 1, origin, width, n_buckets, t_lo, t_hi), f"{origin} {width}")


@pytest.mark.parametrize("mode", layouts.MODES)
def test_layouts_give_the_bytes_of_the_plain_layout(hip, mode):
    batch = layouts.corpus(20_000)[0]
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    args = (first - 33, 37 * INTERVAL, (last - first) // (37 * INTERVAL) + 2)
    plain = hip.m4_buckets(batch, *args)
    if mode == layouts.MODES[0]:
        _assert_cells(plain, _oracle(batch, None, 1, *args), "plain")
    assert hip.m4_buckets(layouts.relayout(batch, mode, 7), *args).tobytes() == plain.tobytes()


def test_errors_leave_the_cells_untouched(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, length=2000)
    rng = np.random.default_rng(9)
    cells = np.frombuffer(rng.bytes(3 * 10 * mdb.M4_CELL_DTYPE.itemsize), dtype=mdb.M4_CELL_DTYPE).reshape(3, 10).copy()
    before = cells.copy()
    resident = hip.upload_segments(batch)
    seg = batch.as_c()
    group_pointer = groups.ctypes.data_as(ctypes.c_void_p)
    for origin, width, n_groups, which_mask, message in ((0, 100, 3, 1, b"which_mask"), (0, 0, 3, 0, b"width"),
                                                         (0, -5, 3, 0, b"width"), (0, 100, 0, 0, b"n_groups")):
        request = _abi.BucketRequestC(origin, width, 10, I64_MIN, I64_MAX, n_groups, which_mask)
        pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
        group_pointers = (ctypes.c_void_p * 1)(group_pointer.value)
        assert hip.lib.mdb_m4_buckets(hip.handle, ctypes.byref(seg), group_pointer, ctypes.byref(request),
                                      cells.ctypes.data_as(ctypes.c_void_p)) == 1
        assert message in hip.lib.mdb_last_error()
        assert hip.lib.mdb_m4_buckets_list(hip.handle, pointers, group_pointers, 1, ctypes.byref(request),
                                           cells.ctypes.data_as(ctypes.c_void_p)) == 1
        assert hip.lib.mdb_m4_buckets_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(request),
                                          cells.ctypes.data_as(ctypes.c_void_p)) == 1   # (fails before cells is touched)
        assert cells.tobytes() == before.tobytes()
    # a group id out of range, on a row the time range leaves out
    bad = groups.copy()
    bad[-1] = 3
    t_hi = int(batch.start_time[len(batch) // 2])
    assert int(batch.start_time[-1]) > t_hi
    for call in (lambda: hip.m4_buckets(batch, 0, 1000, 10, groups=bad, t_hi=t_hi, cells=cells),
                 lambda: hip.m4_buckets_list([batch.slice(0, 5), batch.slice(5, len(batch))], 0, 1000, 10,
                                             groups=[bad[:5], bad[5:]], t_hi=t_hi, cells=cells),
                 lambda: hip.m4_buckets_dev(resident, 0, 1000, 10, groups=bad, t_hi=t_hi, cells=cells)):
        with pytest.raises(mdb.HipError, match="group id"):
            call()
        assert cells.tobytes() == before.tobytes()
    # NULL arguments
    request = _abi.BucketRequestC(0, 100, 10, I64_MIN, I64_MAX, 3, 0)
    data = cells.ctypes.data_as(ctypes.c_void_p)
    assert hip.lib.mdb_m4_buckets(hip.handle, None, None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_m4_buckets(hip.handle, ctypes.byref(seg), None, None, data) == 1
    assert hip.lib.mdb_m4_buckets(hip.handle, ctypes.byref(seg), None, ctypes.byref(request), None) == 1
    assert hip.lib.mdb_m4_buckets(None, ctypes.byref(seg), None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_m4_buckets_dev(hip.handle, None, None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_m4_buckets_list(hip.handle, None, None, 1, ctypes.byref(request), data) == 1
    assert b"NULL" in hip.lib.mdb_last_error()
    assert cells.tobytes() == before.tobytes()
    # an empty batch and no buckets succeed and change nothing
    hip.m4_buckets(batch.slice(0, 0), 0, 100, 10, cells=cells, n_groups=3)
    hip.m4_buckets(batch, 0, 100, 0, groups=groups, cells=np.zeros((3, 0), dtype=mdb.M4_CELL_DTYPE))
    assert cells.tobytes() == before.tobytes()
    resident.free()
