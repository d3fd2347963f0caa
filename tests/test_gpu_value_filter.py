"""Value predicates pushed down to the segments (mdb_grid_*_filter*, mdb_agg_batch_filter*) against the reference's
plan GridExec -> FilterExec (-> AggregateExec): the oracle's grid with the time range and a numpy totalOrder mask on
the values. Rows, values, rows_per_segment and metrics bit for bit; COUNT / MIN / MAX exact, SUM within 0.001 %; the
host, dev and list forms of the aggregates and two runs bit for bit."""

import ctypes
import struct

import numpy as np
import pytest

import cases
import datagen
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM

pytestmark = pytest.mark.gpu

ALL = MDB_AGG_COUNT | MDB_AGG_MIN | MDB_AGG_MAX | MDB_AGG_SUM
SUM_TOLERANCE = 1e-5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
F32_MAX = np.float32(np.finfo(np.float32).max)
EPOCH_US = 1_700_000_000_000_000


@pytest.fixture(scope="module")
def context():
    ctx = mdb.Context(0)
    yield ctx
    ctx.close()


_GRIDS = {}


def _grid(batch):
    key = id(batch)
    if key not in _GRIDS:
        _GRIDS[key] = (batch, ora.grid_batch(batch))
    return _GRIDS[key][1]


def _keys(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def _key_bounds(flt):
    lo_bits, hi_bits = mdb.value_filter_bits(flt)
    lo = -(1 << 31) if flt.flags & 4 else int(_keys(np.uint32(lo_bits).view(np.float32))) + (1 if flt.flags & 1 else 0)
    hi = (1 << 31) - 1 if flt.flags & 8 else int(_keys(np.uint32(hi_bits).view(np.float32))) - (1 if flt.flags & 2 else 0)
    return lo, hi


def _expected(batch, flt):
    """(timestamps, values, rows_per_segment) of ora.grid_batch inside the time range whose value passes."""
    timestamps, values, rows, _ = _grid(batch)
    segment = np.repeat(np.arange(len(batch)), rows.astype(np.int64))
    lo, hi = _key_bounds(flt)
    keys = _keys(values)
    keep = (timestamps >= flt.t_lo) & (timestamps <= flt.t_hi) & (keys >= lo) & (keys <= hi)
    return timestamps[keep], values[keep], np.bincount(segment[keep], minlength=len(batch)).astype(np.uint32)


def _expected_agg(values):
    values = np.asarray(values, dtype=np.float32)
    if len(values) == 0:
        return 0, 0.0, F32_MAX, -F32_MAX, 0.0
    return (len(values), float(np.sum(values.astype(np.float64))), np.fmin.reduce(values, initial=F32_MAX),
            np.fmax.reduce(values, initial=-F32_MAX), float(np.sum(np.abs(values.astype(np.float64)))))


def _same_float(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a == b


def _check_agg(state, expected, what):
    count, total, low, high, magnitude = expected
    assert state.count == count, what
    assert _same_float(state.min, low), (what, state.min, low)
    assert _same_float(state.max, high), (what, state.max, high)
    if not np.isfinite(total) or not np.isfinite(state.sum):
        assert (np.isnan(total) and np.isnan(state.sum)) or total == state.sum, (what, state.sum, total)
    else:
        assert abs(state.sum - total) <= SUM_TOLERANCE * max(magnitude, 1e-300), (what, state.sum, total)


def _state_bits(state):
    return bytes(ctypes.string_at(ctypes.addressof(state), ctypes.sizeof(state)))


def _check_all(context, batch, flt, what, dev=None, with_metrics=True):
    exp_ts, exp_val, exp_rows = _expected(batch, flt)
    got = context.grid_filter(batch, flt)
    cases.assert_grid_equal(got, (exp_ts, exp_val))
    assert np.array_equal(got[2], exp_rows), what
    if with_metrics:
        range_metrics = context.grid_batch_range(batch, flt.t_lo, flt.t_hi)[3]
        metrics = got[3]
        assert metrics["rows_created"] == len(exp_ts)
        for k, name in enumerate(mdb.MODEL_TYPE_NAMES):
            produced = int(exp_rows[batch.model_type_id == k].sum())
            assert metrics[f"rows_created_by_{name}"] == produced, (what, name)
        for key, value in range_metrics.items():
            if not key.startswith("rows_created"):
                assert metrics[key] == value, (what, key)
    owned = dev is None
    if owned:
        dev = context.upload_segments(batch)
    try:
        dev_ts, dev_val, dev_rows, dev_metrics = context.grid_filter_resident(dev, flt)
        cases.assert_grid_equal((dev_ts, dev_val), (exp_ts, exp_val))
        assert np.array_equal(dev_rows, exp_rows) and dev_metrics == got[3], what
        host = context.agg_filter(batch, flt, ALL)
        _check_agg(host, _expected_agg(exp_val), what)
        on_device = context.agg_filter_dev(dev, flt, ALL)
        listed = context.agg_filter_list([batch.take(np.arange(0, len(batch) // 2)),
                                          batch.take(np.arange(len(batch) // 2, len(batch)))], flt, ALL)
        again = context.agg_filter(batch, flt, ALL)
        assert _state_bits(host) == _state_bits(on_device) == _state_bits(listed) == _state_bits(again), what
    finally:
        if owned:
            dev.free()


def _neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def _filters_for(batch, time_ranges):
    """Bounds below / above everything, on a rebuilt value and its f32 neighbours (open and closed), on a segment's
    stored min / max, each with every time range."""
    _, values, _, _ = _grid(batch)
    finite = values[np.isfinite(values)]
    picked = finite[len(finite) // 3] if len(finite) else np.float32(1.0)
    stored = [batch.min_value[len(batch) // 2], batch.max_value[len(batch) // 2]]
    out = [dict(), dict(hi=-1e39), dict(lo=1e39), dict(lo=float(np.min(finite)) if len(finite) else 0.0)]
    for v in _neighbours(picked):
        out += [dict(lo=float(v)), dict(lo=float(v), lo_open=True), dict(hi=float(v)), dict(hi=float(v), hi_open=True),
                dict(lo=float(v), hi=float(v))]
    for v in stored:
        out += [dict(lo=float(v)), dict(hi=float(v), hi_open=True), dict(lo=float(v), hi=float(v) + 50.0)]
    return [dict(bounds, t_lo=t_lo, t_hi=t_hi) for bounds in out for (t_lo, t_hi) in time_ranges]


def _time_ranges(batch):
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    third = (last - first) // 3
    return [(None, None), (first + third, last - third), (first - 5, first + 7 * 100 + 3)]


@pytest.mark.parametrize("eb_name,irregular", [("lossless", False), ("abs5", False), ("rel1", True),
                                               ("abs0.01", True), ("rel5", False)])
def test_mixed_batches_match_the_filtered_grid(context, eb_name, irregular):
    _, _, batch = cases.mixed_batch(cases.error_bounds()[eb_name], irregular, seed=900 + len(eb_name), length=8000)
    dev = context.upload_segments(batch)
    try:
        filters = _filters_for(batch, _time_ranges(batch))
        for k, spec in enumerate(filters):
            flt = mdb.value_filter(**spec)
            _check_all(context, batch, flt, (eb_name, irregular, spec), dev=dev, with_metrics=k % 3 == 0)
    finally:
        dev.free()


def test_edge_cases_nan_inf_and_zeros(context):
    batch = cases.edge_case_batch()
    lossy = cases.edge_case_batch(cases.error_bounds()["abs5"])
    nan, inf = float("nan"), float("inf")
    neg_nan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
    specs = [dict(), dict(lo=0.0), dict(hi=-0.0), dict(lo=-0.0, hi=0.0), dict(lo=0.0, hi=0.0), dict(lo=-0.0, hi=-0.0),
             dict(lo=inf), dict(hi=-inf), dict(lo=nan), dict(hi=neg_nan), dict(lo=-inf, hi=inf),
             dict(lo=0.0, lo_open=True, hi=inf), dict(lo=-1e-45, hi=1e-45), dict(lo=37.0, hi=73.0, hi_open=True),
             dict(lo=3.0, hi=2.0), dict(lo=5.0, hi=5.0, hi_open=True), dict(lo=5.0, t_lo=150, t_hi=950)]
    for which in (batch, lossy):
        for spec in specs:
            _check_all(context, which, mdb.value_filter(**spec), spec)


def test_swing_crossing_zero_and_epoch_timestamps(context):
    """Swing lines that cross zero (the ±0 order of the binary search) and at 1.7e15 us, bounds on the segments'
    stored extremes (the rebuilt points can round past them there)."""
    eb = mdb.error_bound("absolute", 0.5)
    parts = []
    for k, slope in enumerate((1e-3, -1e-3, 2.5e-4, -7e-6)):
        ts = EPOCH_US + np.arange(3000, dtype=np.int64) * 1000 + k
        values = (slope * (np.arange(3000) - 1500.0 - 13.0 * k)).astype(np.float32)
        parts.append(ora.try_compress_univariate_time_series(ts, values, eb))
    ts = np.arange(2000, dtype=np.int64) * 100
    parts.append(ora.try_compress_univariate_time_series(ts, ((np.arange(2000) - 1000) * 1e-3).astype(np.float32), eb))
    batch = mdb.SegmentBatch.concat(parts)
    assert (batch.model_type_id == mdb.MDB_SWING_ID).any()
    specs = [dict(lo=0.0), dict(hi=-0.0), dict(lo=-0.0, hi=0.0), dict(lo=0.0, lo_open=True), dict(hi=0.0, hi_open=True)]
    for i in range(len(batch)):
        for v in (batch.min_value[i], batch.max_value[i]):
            for n in _neighbours(v):
                specs += [dict(lo=float(n)), dict(hi=float(n)), dict(lo=float(n), lo_open=True),
                          dict(hi=float(n), hi_open=True)]
    dev = context.upload_segments(batch)
    try:
        for k, spec in enumerate(specs):
            _check_all(context, batch, mdb.value_filter(**spec), spec, dev=dev, with_metrics=k % 7 == 0)
    finally:
        dev.free()


def test_no_value_bounds_equal_the_range_calls(context):
    for eb_name, irregular in (("rel1", False), ("lossless", True)):
        _, _, batch = cases.mixed_batch(cases.error_bounds()[eb_name], irregular, seed=77, length=6000)
        first, last = int(batch.start_time.min()), int(batch.end_time.max())
        for t_lo, t_hi in ((I64_MIN, I64_MAX), (first + 12345, last - 23456)):
            flt = mdb.value_filter(t_lo=t_lo, t_hi=t_hi)
            got = context.grid_filter(batch, flt)
            expected = context.grid_batch_range(batch, t_lo, t_hi)
            cases.assert_grid_equal(got, expected)
            assert np.array_equal(got[2], expected[2]) and got[3] == expected[3]
            state, ranged = context.agg_filter(batch, flt, ALL), context.agg_batch_range(batch, t_lo, t_hi, ALL)
            assert state.count == ranged.count and _same_float(state.min, ranged.min)
            assert _same_float(state.max, ranged.max)
            assert abs(state.sum - ranged.sum) <= SUM_TOLERANCE * abs(ranged.sum)


def test_several_slices_under_a_scratch_limit(context):
    _, _, lossless = cases.mixed_batch(cases.LOSSLESS, True, seed=31, length=20_000)
    _, _, lossy = cases.mixed_batch(cases.error_bounds()["rel1"], False, seed=32, length=20_000)
    batch = mdb.SegmentBatch.concat([lossless, lossy])
    _, values, _, _ = _grid(batch)
    ctx = mdb.Context(0)
    try:
        ctx.set_scratch_limit(1 << 16)  # slices of 1365 points
        for spec in (dict(lo=float(np.median(values))), dict(), dict(hi=float(values[5]), t_lo=int(batch.start_time[3]))):
            _check_all(ctx, batch, mdb.value_filter(**spec), spec, with_metrics=False)
    finally:
        ctx.close()


def test_errors_leave_the_outputs_untouched(context):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["abs5"], False, seed=5, length=3000)
    good = mdb.value_filter(lo=150.0)
    bad_flags = mdb.value_filter(lo=1.0)
    bad_flags.flags |= 16
    bad_reserved = mdb.value_filter(lo=1.0)
    bad_reserved.reserved = 1
    before = _state_bits(mdb._abi.AggStateC(1.5, 3, 2.0, 4.0))
    dev = context.upload_segments(batch)
    try:
        for bad in (bad_flags, bad_reserved):
            for call in (lambda state: context.agg_filter(batch, bad, ALL, state),
                         lambda state: context.agg_filter_list([batch], bad, ALL, state),
                         lambda state: context.agg_filter_dev(dev, bad, ALL, state)):
                state = mdb._abi.AggStateC(1.5, 3, 2.0, 4.0)
                with pytest.raises(mdb.HipError):
                    call(state)
                assert _state_bits(state) == before
            with pytest.raises(mdb.HipError):
                context.grid_filter(batch, bad)
            with pytest.raises(mdb.HipError):
                context.grid_count_filter_dev(dev, bad)
        n = context.grid_count_filter_dev(dev, good)
        assert n > 1
        out_ts, out_val = context.dev_alloc(8 * n), context.dev_alloc(4 * n)
        try:
            n_out = ctypes.c_uint64(12345)
            metrics = mdb._abi.GridMetricsC()
            for flt, cap in ((good, n - 1), (bad_flags, n)):
                code = context.lib.mdb_grid_batch_filter_dev(context.handle, ctypes.byref(dev.seg), ctypes.byref(flt),
                                                             ctypes.c_void_p(out_ts), ctypes.c_void_p(out_val), None,
                                                             cap, ctypes.byref(n_out), ctypes.byref(metrics))
                assert code != 0 and n_out.value == 12345 and metrics.rows_created == 0
        finally:
            context.dev_free(out_ts)
            context.dev_free(out_val)
    finally:
        dev.free()


def test_untouched_device_outputs_on_cap_error(context):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["abs5"], False, seed=6, length=3000)
    flt = mdb.value_filter(lo=120.0)
    dev = context.upload_segments(batch)
    try:
        n = context.grid_count_filter_dev(dev, flt)
        sentinel_ts = np.full(n, -7, dtype=np.int64)
        sentinel_val = np.full(n, 0x5A5A5A5A, dtype=np.uint32).view(np.float32)
        out_ts, out_val = context.upload_array(sentinel_ts), context.upload_array(sentinel_val)
        try:
            with pytest.raises(mdb.HipError):
                context.grid_filter_dev(dev, flt, out_ts, out_val, n - 1)
            assert np.array_equal(context.download_array(out_ts, n, np.int64), sentinel_ts)
            assert np.array_equal(context.download_array(out_val, n, np.float32).view(np.uint32),
                                  sentinel_val.view(np.uint32))
        finally:
            context.dev_free(out_ts)
            context.dev_free(out_val)
    finally:
        dev.free()


def test_empty_batch_and_nothing_passing(context):
    _, _, batch = cases.mixed_batch(cases.error_bounds()["abs5"], False, seed=8, length=2000)
    nothing = mdb.value_filter(lo=5.0, hi=5.0, hi_open=True)
    state = context.agg_filter(batch, nothing, ALL, mdb._abi.AggStateC(0.0, 0, float("nan"), float("nan")))
    ranged = context.agg_batch_range(batch, 10**18, 10**18 + 1, ALL, mdb._abi.AggStateC(0.0, 0, float("nan"),
                                                                                             float("nan")))
    assert _state_bits(state) == _state_bits(ranged)
    ts, values, rows, metrics = context.grid_filter(batch, nothing, reserve_front=5)
    assert len(ts) == len(values) == 0 and not rows.any() and metrics["rows_created"] == 0
    empty = batch.take(np.arange(0))
    assert len(context.grid_filter(empty, nothing)[0]) == 0
    state = context.agg_filter(empty, nothing, ALL)
    assert (state.count, state.sum) == (0, 0.0)


def test_seeded_fuzz(context):
    rng = np.random.default_rng(2026)
    bounds = list(cases.error_bounds().values())
    for trial in range(12):
        eb = bounds[int(rng.integers(len(bounds)))]
        timestamps, values = datagen.generate_univariate_time_series(
            int(rng.integers(50, 3000)), (int(rng.integers(2, 60)), int(rng.integers(61, 400))), bool(rng.integers(2)),
            (1.0, 1.0 + float(rng.uniform(0, 0.2))), (float(rng.uniform(-100, 0)), float(rng.uniform(1, 100))),
            int(rng.integers(1 << 30)))
        batch = ora.try_compress_univariate_time_series(timestamps, values, eb)
        _, grid_values, _, _ = _grid(batch)
        pick = lambda: float(grid_values[int(rng.integers(len(grid_values)))]) if len(grid_values) else 0.0
        lo, hi = sorted([pick(), pick()])
        spec = dict(lo=lo if rng.integers(3) else None, hi=hi if rng.integers(3) else None,
                    lo_open=bool(rng.integers(2)), hi_open=bool(rng.integers(2)))
        if rng.integers(2):
            a, b = sorted(rng.integers(int(timestamps[0]) - 10, int(timestamps[-1]) + 10, 2).tolist())
            spec.update(t_lo=a, t_hi=b)
        _check_all(context, batch, mdb.value_filter(**spec), (trial, spec), with_metrics=trial % 3 == 0)
