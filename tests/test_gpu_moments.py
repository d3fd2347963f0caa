"""Variance and standard deviation on segments (mdb_moments_buckets*): per date_bin bucket and group the count, the
mean and m2 = sum((v - mean)^2). The reference is ora.grid_batch's points, put into cells as tests/test_gpu_m4.py's
oracle does, and per cell in exact arithmetic (math.fsum): d = v - v[0] in f64, mean_ref = v[0] + fsum(d) / n,
m2_ref = fsum((d - fsum(d) / n)^2).

Tolerances: count exact; |mean - mean_ref| <= 2^-44 * max|v| of the cell (the f64 unit roundoff with a margin of 2^9
for the merges); |m2 - m2_ref| <= 1e-5 * m2_ref - so a cell of equal values has m2 == 0.0 exactly. In a cell that
holds a NaN or an infinity neither mean nor m2 is finite, and nothing more is asked."""

import ctypes
import math

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
SUM_TOLERANCE = 1e-5          # tests/test_gpu_agg_buckets.py's, for SUM / COUNT against mean


from moments_cases import (GRIDS as _GRIDS, MEAN_TOLERANCE, M2_TOLERANCE, point_buckets as _point_buckets, grid as _grid,
                           cell_reference as _cell_reference, reduce as _reduce, oracle as _oracle,
                           assert_cells as _assert_cells)


def _series_batch(eb, irregular, n_series=3, length=6000, seed=400):
    parts = [cases.mixed_batch(eb, irregular, seed=seed + k, length=length)[2] for k in range(n_series)]
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    return mdb.SegmentBatch.concat(parts), groups


def _bucket_sets(first, last):
    """(name, origin, width, n_buckets, t_lo, t_hi) over data in [first, last]: those of tests/test_gpu_m4.py."""
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


_SHARED = {}


def _rel5_batch():
    """The rel5 / regular batch of the parity test with its groups: shared by the tests that need some batch."""
    if "rel5" not in _SHARED:
        _SHARED["rel5"] = _series_batch(cases.error_bounds()["rel5"], False)
    return _SHARED["rel5"]


@pytest.mark.parametrize("eb_name", ["lossless", "rel5", "abs5"])
@pytest.mark.parametrize("irregular", [False, True], ids=["regular", "irregular"])
def test_parity_with_the_points_in_exact_arithmetic(hip, eb_name, irregular):
    batch, groups = (_rel5_batch() if (eb_name, irregular) == ("rel5", False)
                     else _series_batch(cases.error_bounds()[eb_name], irregular))
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    for name, origin, width, n_buckets, t_lo, t_hi in _bucket_sets(first, last):
        got = hip.moments_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
        _assert_cells(got, _oracle(batch, groups, 3, origin, width, n_buckets, t_lo, t_hi), f"{eb_name} {name}")


@pytest.mark.parametrize("eb_name", ["lossless", "rel5"])
def test_edge_case_series(hip, eb_name):
    """NaN, infinities, one- and two-point segments, long residual tails, huge timestamp gaps: each series a group."""
    eb = cases.error_bounds()[eb_name]
    parts = [ora.try_compress_univariate_time_series(ts, v, eb) for _, ts, v in cases.edge_case_series()]
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    batch = mdb.SegmentBatch.concat(parts)
    special = 0
    for origin, width, n_buckets in ((0, 100, 40), (-35, 250, 24), (1658671178037 - 1000, 3000, 30), (0, 1 << 40, 3)):
        got = hip.moments_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=len(parts))
        expected = _oracle(batch, groups, len(parts), origin, width, n_buckets)
        _assert_cells(got, expected, f"{eb_name} {origin} {width}")
        special += int(((expected["count"] > 0) & ~expected["finite"]).sum())
    assert special > 0   # (cells with a NaN or an infinity were among them)


def _conditioning_series():
    """(name, values): a sensor at level 1e6 with sigma 0.5, and one at 1e7 that flips between two adjacent f32."""
    rng = np.random.default_rng(1206)
    n = 20_000
    noisy = (1.0e6 + rng.normal(0.0, 0.5, n)).astype(np.float32)
    low = np.float32(1.0e7)
    flipping = np.where(rng.random(n) < 0.5, low, np.nextafter(low, np.float32(np.inf))).astype(np.float32)
    return [("level_1e6_sigma_0.5", noisy), ("level_1e7_one_ulp", flipping)]


@pytest.mark.parametrize("which", [0, 1], ids=["level_1e6_sigma_0.5", "level_1e7_one_ulp"])
def test_conditioning_where_a_sum_of_squares_fails(hip, which):
    """Shifted sums keep m2 within 1e-5 where f64 sum(v^2) - sum(v)^2 / n does not (1.3e-4 and 2.7e-2 relative on
    series like these): the second half of the test holds the algorithm to that choice."""
    name, values = _conditioning_series()[which]
    n = len(values)
    timestamps = np.arange(n, dtype=np.int64) * INTERVAL
    batch = ora.try_compress_univariate_time_series(timestamps, values, cases.LOSSLESS)
    np.testing.assert_array_equal(_grid(batch)[1].view(np.uint32), values.view(np.uint32))   # (lossless)
    for origin, width, n_buckets in ((0, n * INTERVAL, 1), (0, 7 * INTERVAL, n // 7 + 1)):
        got = hip.moments_buckets(batch, origin, width, n_buckets)
        _assert_cells(got, _oracle(batch, None, 1, origin, width, n_buckets), f"{name} {n_buckets} bucket(s)")
    wide = values.astype(np.float64)
    naive = float(np.sum(wide * wide) - np.sum(wide) ** 2 / n)
    m2_ref = _cell_reference(values)[1]
    print(f"{name}: sum of squares misses m2 by {abs(naive - m2_ref) / m2_ref:.3g} relative")
    assert abs(naive - m2_ref) > M2_TOLERANCE * m2_ref


def test_constant_cells_have_no_variance(hip):
    """PMC-Mean segments only, several of one value per bucket: m2 == 0.0 and mean == the value exactly, in pair order
    and shuffled (the sort path), in buckets and in one bucket."""
    levels = np.array([1234.567, -0.1, 1.0e7 + 1.0], dtype=np.float32)
    parts, groups = [], []
    for g, level in enumerate(levels):
        for k in range(12):
            timestamps = (np.arange(50, dtype=np.int64) + 50 * k) * INTERVAL
            part = ora.try_compress_univariate_time_series(timestamps, np.full(50, level, dtype=np.float32), cases.LOSSLESS)
            assert (part.model_type_id == mdb.MDB_PMC_MEAN_ID).all()
            parts.append(part)
            groups.append(np.full(len(part), g, dtype=np.uint32))
    batch, groups = mdb.SegmentBatch.concat(parts), np.concatenate(groups)
    order = np.random.default_rng(3).permutation(len(batch))
    for origin, width, n_buckets in ((0, 170 * INTERVAL, 4), (-30, 600 * INTERVAL + 30, 1), (0, 7 * INTERVAL, 86)):
        for rows, ids in ((batch, groups), (batch.take(order), groups[order])):
            got = hip.moments_buckets(rows, origin, width, n_buckets, groups=ids, n_groups=3)
            assert (got["count"] > 0).all() and int(got["count"].sum()) == 3 * 600
            assert (got["m2"] == 0.0).all() and not np.signbit(got["m2"]).any()
            assert (got["mean"] == levels.astype(np.float64)[:, None]).all()
    # (more than one segment of 50 points in every cell)
    assert (hip.moments_buckets(batch, 0, 170 * INTERVAL, 4, groups=groups, n_groups=3)["count"] > 50).all()


def test_forms_and_runs_agree_bit_for_bit(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, n_series=4, length=6000, seed=420)
    lossless, lossless_groups = _series_batch(cases.LOSSLESS, True, n_series=2, length=4000, seed=430)
    batch = mdb.SegmentBatch.concat([batch, lossless])
    groups = np.concatenate([groups, lossless_groups + 4])
    args = (-777, 1_300, 500)
    first = hip.moments_buckets(batch, *args, groups=groups, n_groups=6)
    _assert_cells(first, _oracle(batch, groups, 6, *args), "host form")
    assert hip.moments_buckets(batch, *args, groups=groups, n_groups=6).tobytes() == first.tobytes()
    assert hip.moments_buckets_list([batch], *args, groups=[groups], n_groups=6).tobytes() == first.tobytes()
    resident = hip.upload_segments(batch)
    on_device = hip.moments_buckets_dev(resident, *args, groups=groups, n_groups=6)
    assert on_device.tobytes() == first.tobytes()
    assert hip.moments_buckets_dev(resident, *args, groups=groups, n_groups=6).tobytes() == first.tobytes()
    resident.free()


def test_order_and_slicing_stay_within_the_tolerance(hip, monkeypatch):
    """What changes the order of the merges moves the cells by rounding only: each variant is held to the same
    reference with the same tolerance."""
    batch, groups = _rel5_batch()
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    args = (first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2)
    expected = _oracle(batch, groups, 3, *args)
    cuts = list(range(0, len(batch), 3)) + [len(batch)]
    listed = hip.moments_buckets_list([batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])], *args,
                                      groups=[groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])], n_groups=3)
    _assert_cells(listed, expected, "list entries of three segments")
    half = len(batch) // 2
    halves = ((0, half), (half, len(batch)))
    for name, (one, other) in (("first half, then second", halves), ("second half, then first", halves[::-1])):
        cells = hip.moments_buckets(batch.slice(*one), *args, groups=groups[one[0]:one[1]], n_groups=3)
        separately = hip.moments_buckets(batch.slice(*other), *args, groups=groups[other[0]:other[1]], n_groups=3)
        merged = mdb.moments_merge(cells.copy(), separately)
        cells = hip.moments_buckets(batch.slice(*other), *args, groups=groups[other[0]:other[1]], cells=cells)
        _assert_cells(cells, expected, name)
        assert merged.tobytes() == cells.tobytes()   # (the host's merge rule is the kernels')
    order = np.random.default_rng(6).permutation(len(batch))
    shuffled = hip.moments_buckets(batch.take(order), *args, groups=groups[order], n_groups=3)
    _assert_cells(shuffled, expected, "shuffled (sort path)")
    one_group = hip.moments_buckets(batch, *args)   # (keys out of order across series: the sort path, too)
    _assert_cells(one_group, _oracle(batch, None, 1, *args), "one group")
    wide = (first, last - first + 1, 1)             # (every pair of a series in one cell: runs through the tree)
    monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "1000")
    sliced = hip.moments_buckets(batch, *args, groups=groups, n_groups=3)
    sliced_wide = hip.moments_buckets(batch, *wide, groups=groups, n_groups=3)
    monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
    _assert_cells(sliced, expected, "slices of 1000 pairs")
    _assert_cells(sliced_wide, _oracle(batch, groups, 3, *wide), "slices of 1000 pairs, one bucket")


def test_runs_of_one_cell_through_every_level_of_the_reduction_tree(hip):
    """More than 4 096 pairs in one cell: level 0's tiles, then levels 1 and 2."""
    base, _ = _series_batch(cases.error_bounds()["rel5"], False, n_series=1, length=6000, seed=440)
    big = base.take(np.tile(np.arange(len(base)), 5000 // len(base) + 2))
    assert len(big) > 4096
    first, last = int(big.start_time.min()), int(big.end_time.max())
    for width, n_buckets in ((last - first + 1, 1), ((last - first) // 2 + 1, 2)):
        got = hip.moments_buckets(big, first, width, n_buckets)
        _assert_cells(got, _oracle(big, None, 1, first, width, n_buckets), f"{n_buckets} bucket(s)")


def test_macaque_v_through_the_cursor_index_and_without(hip, monkeypatch):
    """Lossless MacaqueV streams of 65 536 values, regular and irregular timestamps: piece by piece from the cursor
    index (k_moments_pieces), and one lane per stream with MDB_GRID_MV_INDEX=0."""
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
            got = hip.moments_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=2)
            kernels = hip.profile()
            assert "k_moments_pieces" in kernels and "k_moments_partials" in kernels, sorted(kernels)
            _assert_cells(got, expected, f"index {width}")
            on_device = hip.moments_buckets_dev(resident, origin, width, n_buckets, groups=groups, n_groups=2)
            assert on_device.tobytes() == got.tobytes()
            monkeypatch.setenv("MDB_GRID_MV_INDEX", "0")
            hip.profile_reset()
            serial = hip.moments_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=2)
            kernels = hip.profile()
            monkeypatch.delenv("MDB_GRID_MV_INDEX")
            assert "k_moments_pieces" not in kernels and "k_moments_partials" in kernels, sorted(kernels)
            _assert_cells(serial, expected, f"no index {width}")
    finally:
        hip.profile_enable(False)
        resident.free()


def _layout_requests(batch):
    """Two requests of 37 intervals a bucket over the layouts corpus, in front of and behind its gap of 2^40 (one
    request over both would have 6e8 buckets): the mixed series with their NaN / infinity edge cases, and the residual
    tails and long MacaqueV streams."""
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    behind = batch.start_time > first + (1 << 41)
    assert 20 < int(behind.sum()) < len(batch) - 20
    front_last = int(batch.end_time[batch.end_time < first + (1 << 40)].max())   # (not the rows that span the gap)
    behind_first = int(batch.start_time[behind].min())
    width = 37 * INTERVAL
    requests = [(first - 33, width, (front_last - first) // width + 2),
                (behind_first - 33, width, (last - behind_first) // width + 2)]
    assert all(n_buckets < 5_000 for _, _, n_buckets in requests), requests
    return requests


@pytest.mark.parametrize("mode", ["three", "padded-one"])
def test_layouts_give_the_bytes_of_the_plain_layout(hip, mode):
    """A multi-buffer and a padded BinaryView layout of the layouts corpus."""
    assert mode in layouts.MODES
    batch = layouts.corpus(20_000)[0]
    moved = layouts.relayout(batch, mode, 7)
    for k, args in enumerate(_layout_requests(batch)):
        if ("plain", k) not in _SHARED:
            _SHARED["plain", k] = hip.moments_buckets(batch, *args)
            _assert_cells(_SHARED["plain", k], _oracle(batch, None, 1, *args), f"plain {k}")
            assert int((_SHARED["plain", k]["count"] > 0).sum()) > 100
        assert hip.moments_buckets(moved, *args).tobytes() == _SHARED["plain", k].tobytes()


def test_relation_to_agg_buckets(hip):
    batch, groups = _rel5_batch()
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    for name, origin, width, n_buckets, t_lo, t_hi in _bucket_sets(first, last)[1:]:
        cells = hip.moments_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
        states = hip.agg_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
        np.testing.assert_array_equal(cells["count"], states["count"])
        hit = cells["count"] > 0
        assert np.isfinite(cells["mean"][hit]).all()
        average = states["sum"][hit] / states["count"][hit]
        assert (np.abs(cells["mean"][hit] - average) <= SUM_TOLERANCE * np.abs(average)).all(), name
    # with non-finite points in the cells: the counts still agree
    batch = cases.edge_case_batch()
    cells = hip.moments_buckets(batch, -35, 250, 24)
    np.testing.assert_array_equal(cells["count"], hip.agg_buckets(batch, -35, 250, 24)["count"])


def test_cells_that_receive_nothing_keep_their_bytes(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, length=2000)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    origin, width, n_buckets = first - 10 * 3_000, 3_000, (last - first) // 3_000 + 30
    expected = _oracle(batch, groups, 4, origin, width, n_buckets)   # (group 3 has no segment)
    empty = expected["count"] == 0
    assert empty[:3].any() and empty[3].all() and (~empty).any()
    cells = mdb.fresh_moments_cells((4, n_buckets))
    cells.view(np.uint8).reshape(4, n_buckets, -1)[empty] = 0xA5
    pattern = cells.copy()
    resident = hip.upload_segments(batch)
    for form in ("host", "dev"):
        got = cells.copy()
        if form == "host":
            hip.moments_buckets(batch, origin, width, n_buckets, groups=groups, cells=got)
        else:
            hip.moments_buckets_dev(resident, origin, width, n_buckets, groups=groups, cells=got)
        assert got[empty].tobytes() == pattern[empty].tobytes(), form
        filled = got.copy()
        filled[empty] = 0
        _assert_cells(filled, expected, form)
    resident.free()


def test_the_ungrouped_in_time_convenience_and_the_variance(hip):
    """Context.moments is one bucket over the data inside the range; moments_variance gives numpy's var of it."""
    batch, groups = _rel5_batch()
    timestamps, values, rows = _grid(batch)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    point_groups = np.repeat(groups.astype(np.int64), rows)
    for t_lo, t_hi in ((None, None), (first + 7_777, last - 12_321), (last + 1, None)):
        cells = hip.moments(batch, t_lo, t_hi, groups=groups)
        assert cells.shape == (3,)
        keep = (timestamps >= (I64_MIN if t_lo is None else t_lo)) & (timestamps <= (I64_MAX if t_hi is None else t_hi))
        for ddof in (0, 1):
            variance = mdb.moments_variance(cells, ddof)
            for g in range(3):
                points = values[keep & (point_groups == g)].astype(np.float64)
                assert cells["count"][g] == len(points)
                if len(points) > ddof:
                    assert abs(variance[g] - np.var(points, ddof=ddof)) <= 1e-9 * np.var(points, ddof=ddof)
                else:
                    assert np.isnan(variance[g])


def test_errors_leave_the_cells_untouched(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, length=2000)
    rng = np.random.default_rng(9)
    size = mdb.MOMENTS_CELL_DTYPE.itemsize
    cells = np.frombuffer(rng.bytes(3 * 10 * size), dtype=mdb.MOMENTS_CELL_DTYPE).reshape(3, 10).copy()
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
        assert hip.lib.mdb_moments_buckets(hip.handle, ctypes.byref(seg), group_pointer, ctypes.byref(request), data) == 1
        assert message in hip.lib.mdb_last_error()
        assert hip.lib.mdb_moments_buckets_list(hip.handle, pointers, group_pointers, 1, ctypes.byref(request), data) == 1
        assert message in hip.lib.mdb_last_error()
        # (fails before `data`, a host pointer here, is touched)
        assert hip.lib.mdb_moments_buckets_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(request), data) == 1
        assert message in hip.lib.mdb_last_error()
        assert cells.tobytes() == before.tobytes()
    # a group id out of range, on a row the time range leaves out
    bad = groups.copy()
    bad[-1] = 3
    t_hi = int(batch.start_time[len(batch) // 2])
    assert int(batch.start_time[-1]) > t_hi
    for call in (lambda: hip.moments_buckets(batch, 0, 1000, 10, groups=bad, t_hi=t_hi, cells=cells),
                 lambda: hip.moments_buckets_list([batch.slice(0, 5), batch.slice(5, len(batch))], 0, 1000, 10,
                                                  groups=[bad[:5], bad[5:]], t_hi=t_hi, cells=cells),
                 lambda: hip.moments_buckets_dev(resident, 0, 1000, 10, groups=bad, t_hi=t_hi, cells=cells)):
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
    for call in (lambda: hip.moments_buckets(broken, origin, width, 10, groups=groups, cells=cells),
                 lambda: hip.moments_buckets_dev(broken_resident, origin, width, 10, groups=groups, cells=cells)):
        with pytest.raises(mdb.HipError, match="model type"):
            call()
        assert cells.tobytes() == before.tobytes()
    broken_resident.free()
    # NULL arguments
    request = _abi.BucketRequestC(0, 100, 10, I64_MIN, I64_MAX, 3, 0)
    assert hip.lib.mdb_moments_buckets(hip.handle, None, None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_moments_buckets(hip.handle, ctypes.byref(seg), None, None, data) == 1
    assert hip.lib.mdb_moments_buckets(hip.handle, ctypes.byref(seg), None, ctypes.byref(request), None) == 1
    assert hip.lib.mdb_moments_buckets(None, ctypes.byref(seg), None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_moments_buckets_dev(hip.handle, None, None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_moments_buckets_list(hip.handle, None, None, 1, ctypes.byref(request), data) == 1
    assert b"NULL" in hip.lib.mdb_last_error()
    assert cells.tobytes() == before.tobytes()
    resident.free()


def test_empty_input_succeeds_and_changes_nothing(hip):
    batch, groups = _rel5_batch()
    rng = np.random.default_rng(10)
    size = mdb.MOMENTS_CELL_DTYPE.itemsize
    cells = np.frombuffer(rng.bytes(3 * 10 * size), dtype=mdb.MOMENTS_CELL_DTYPE).reshape(3, 10).copy()
    before = cells.copy()
    hip.moments_buckets(batch.slice(0, 0), 0, 100, 10, cells=cells, n_groups=3)
    hip.moments_buckets_list([], 0, 100, 10, cells=cells, n_groups=3)
    assert cells.tobytes() == before.tobytes()
    none = np.zeros((3, 0), dtype=mdb.MOMENTS_CELL_DTYPE)
    assert hip.moments_buckets(batch, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    resident = hip.upload_segments(batch)
    assert hip.moments_buckets_dev(resident, 0, 100, 0, groups=groups, cells=none).shape == (3, 0)
    resident.free()
