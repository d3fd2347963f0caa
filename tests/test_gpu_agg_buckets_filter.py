"""COUNT / MIN / MAX / SUM per date_bin bucket and group of the points that pass a value predicate
(mdb_agg_buckets_filter*) against the reference's fallback plan GridExec -> FilterExec -> date_bin -> GROUP BY, restated
two ways: (a) the oracle's grid, the two time ranges, a numpy totalOrder mask on the values and numpy bucketing; (b) for
small cases, mdb_agg_batch_filter per cell (an independent GPU path) over the bucket's bounds. COUNT / MIN / MAX exact,
SUM within 0.001 %; the host, dev and list forms and two runs bit for bit."""

import ctypes as C

import numpy as np
import pytest

import cases
import datagen
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM, _abi

pytestmark = pytest.mark.gpu

ALL = MDB_AGG_COUNT | MDB_AGG_MIN | MDB_AGG_MAX | MDB_AGG_SUM
SUM_TOLERANCE = 1e-5
INTERVAL = 100  # the sampling interval of tests/datagen.py
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
F32_MAX = np.float32(np.finfo(np.float32).max)
EPOCH_US = 1_700_000_000_000_000

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


def _bucket_ids(timestamps, origin, width):
    """floor((ts - origin) / width) with Python integers where int64 could overflow."""
    if len(timestamps) == 0:
        return np.zeros(0, dtype=object)
    if -(1 << 62) < int(timestamps.min()) - origin and int(timestamps.max()) - origin < (1 << 62):
        return np.floor_divide(timestamps - np.int64(origin), np.int64(width)).astype(object)
    return np.array([(int(t) - origin) // width for t in timestamps], dtype=object)


def _oracle(batch, groups, n_groups, origin, width, n_buckets, flt, t_lo=I64_MIN, t_hi=I64_MAX, magnitudes=None):
    """(a): the points of ora.grid_batch inside both time ranges whose value passes, bucketed with numpy. `magnitudes`
    (a list): receives the sum of |value| per cell."""
    timestamps, values, rows, _ = _grid(batch)
    groups = np.zeros(len(batch), dtype=np.uint32) if groups is None else groups
    point_groups = np.repeat(groups.astype(np.int64), rows.astype(np.int64))
    lo_key, hi_key = _key_bounds(flt)
    keys = _keys(values)
    keep = (timestamps >= max(t_lo, flt.t_lo)) & (timestamps <= min(t_hi, flt.t_hi)) & (keys >= lo_key) & (keys <= hi_key)
    buckets = _bucket_ids(timestamps, origin, width)
    keep &= np.array([0 <= b < n_buckets for b in buckets], dtype=bool) if len(buckets) else np.zeros(0, dtype=bool)
    cells = point_groups[keep] * n_buckets + buckets[keep].astype(np.int64)
    picked = values[keep].astype(np.float32)
    n_cells = n_groups * n_buckets
    out = mdb.fresh_agg_states(n_cells)
    counts = np.bincount(cells, minlength=n_cells)
    sums = np.zeros(n_cells)
    with np.errstate(invalid="ignore"):  # (+inf and -inf in one cell: NaN, as in the plan)
        np.add.at(sums, cells, picked.astype(np.float64))
    mins = np.full(n_cells, F32_MAX, dtype=np.float32)
    maxs = np.full(n_cells, -F32_MAX, dtype=np.float32)
    np.fmin.at(mins, cells, picked)
    np.fmax.at(maxs, cells, picked)
    if magnitudes is not None:
        magnitude = np.zeros(n_cells)
        np.add.at(magnitude, cells, np.abs(picked.astype(np.float64)))
        magnitudes.append(magnitude.reshape(n_groups, n_buckets))
    hit = counts > 0
    out["count"][hit], out["sum"][hit], out["min"][hit], out["max"][hit] = counts[hit], sums[hit], mins[hit], maxs[hit]
    return out.reshape(n_groups, n_buckets)


def _with_time(flt, t_lo, t_hi):
    copy = _abi.ValueFilterC.from_buffer_copy(flt)
    copy.t_lo, copy.t_hi = t_lo, t_hi
    return copy


def _oracle_by_filtered_aggregates(hip, batch, groups, n_groups, origin, width, n_buckets, flt, t_lo=I64_MIN,
                                   t_hi=I64_MAX):
    """(b): cell (g, b) is mdb_agg_batch_filter on group g's rows with the filter's time range narrowed to bucket b and
    both ranges."""
    out = mdb.fresh_agg_states((n_groups, n_buckets))
    groups = np.zeros(len(batch), dtype=np.uint32) if groups is None else groups
    for g in range(n_groups):
        rows = np.nonzero(groups == g)[0]
        if len(rows) == 0:
            continue
        part = batch.take(rows)
        for b in range(n_buckets):
            lo = max(origin + b * width, t_lo, flt.t_lo)
            hi = min(origin + (b + 1) * width - 1, t_hi, flt.t_hi, I64_MAX)
            if lo > hi:
                continue
            state = hip.agg_filter(part, _with_time(flt, lo, hi), ALL)
            out[g, b] = (state.sum, state.count, state.min, state.max)
    return out


def _assert_cells(got, expected, context="", magnitude=None):
    """`magnitude` (sum of |value| per cell): for cells whose points cancel - the closed forms of Swing are held to 1e-6
    of each segment's part, not of the cell's total. MIN / MAX bit for bit, but for a cell holding both +0.0 and -0.0:
    which zero is its extreme depends on the order the points are folded in, in the plan as here."""
    assert got.shape == expected.shape
    np.testing.assert_array_equal(got["count"], expected["count"], err_msg=str(context))
    for field in ("min", "max"):
        same = (got[field].view(np.uint32) == expected[field].view(np.uint32)) | ((got[field] == 0) & (expected[field] == 0))
        assert same.all(), (context, field, got[field][~same], expected[field][~same])
    finite = np.isfinite(expected["sum"])
    assert np.array_equal(got["sum"][~finite], expected["sum"][~finite], equal_nan=True), context
    diff = np.abs(got["sum"][finite] - expected["sum"][finite])
    bound = SUM_TOLERANCE * np.maximum(np.abs(expected["sum"][finite]), 1e-30)
    if magnitude is not None:
        bound = bound + 1e-6 * magnitude[finite]
    assert np.all(diff <= bound), (context, float(np.max(diff - bound)))


def _check(hip, batch, groups, n_groups, origin, width, n_buckets, flt, t_lo=I64_MIN, t_hi=I64_MAX, context=""):
    got = hip.agg_buckets_filter(batch, flt, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi,
                                 n_groups=n_groups)
    magnitudes = []
    expected = _oracle(batch, groups, n_groups, origin, width, n_buckets, flt, t_lo, t_hi, magnitudes)
    _assert_cells(got, expected, context, magnitudes[0])
    return got


def _series_batch(eb, irregular, n_series=3, length=6000, seed=400):
    parts = [cases.mixed_batch(eb, irregular, seed=seed + k, length=length)[2] for k in range(n_series)]
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    return mdb.SegmentBatch.concat(parts), groups


def _predicates(batch):
    """>, >=, <, <=, BETWEEN, = c and an empty interval on values the batch rebuilds to, and >= with a time range."""
    _, values, _, _ = _grid(batch)
    finite = np.sort(values[np.isfinite(values)])
    q = lambda f: float(finite[int(f * (len(finite) - 1))])
    unique, counts = np.unique(finite, return_counts=True)
    common = float(unique[np.argmax(counts)])
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    third = (last - first) // 3
    return [
        ("gt", mdb.value_filter(lo=q(0.5), lo_open=True)),
        ("ge", mdb.value_filter(lo=q(0.5))),
        ("lt", mdb.value_filter(hi=q(0.25), hi_open=True)),
        ("le", mdb.value_filter(hi=q(0.75))),
        ("between", mdb.value_filter(lo=q(0.25), hi=q(0.75))),
        ("eq", mdb.value_filter(lo=common, hi=common)),
        ("empty", mdb.value_filter(lo=q(0.5), hi=q(0.5), hi_open=True)),
        ("ge_timed", mdb.value_filter(lo=q(0.4), t_lo=first + third, t_hi=last + 1000)),
    ]


def _bucket_sets(first, last):
    """(name, origin, width, n_buckets, t_lo, t_hi) over data in [first, last]."""
    span = last - first + 1
    return [
        ("width_1_interval", first, INTERVAL, span // INTERVAL + 1, I64_MIN, I64_MAX),
        ("width_7_intervals", first - 33, 7 * INTERVAL, span // (7 * INTERVAL) + 2, I64_MIN, I64_MAX),
        ("width_1000_intervals", first, 1000 * INTERVAL, span // (1000 * INTERVAL) + 1, I64_MIN, I64_MAX),
        ("one_bucket", first, span, 1, I64_MIN, I64_MAX),
        ("range_cuts_buckets", first - 50, 5_000, span // 5_000 + 2, first + 7_777, last - (last - first) // 2),
    ]


@pytest.mark.parametrize("eb_name,irregular", [("lossless", False), ("lossless", True), ("rel5", False),
                                               ("abs5", True), ("rel1", False)])
def test_parity_with_the_filtered_fallback_plan(hip, eb_name, irregular):
    batch, groups = _series_batch(cases.error_bounds()[eb_name], irregular)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    for predicate, flt in _predicates(batch):
        for name, origin, width, n_buckets, t_lo, t_hi in _bucket_sets(first, last):
            _check(hip, batch, groups, 3, origin, width, n_buckets, flt, t_lo, t_hi, (eb_name, predicate, name))
        # one group over all series: keys out of order across series (the sort path)
        _check(hip, batch, None, 1, first, 7 * INTERVAL, (last - first) // (7 * INTERVAL) + 1, flt,
               context=(eb_name, predicate, "one group"))


@pytest.mark.parametrize("eb_name,irregular", [("rel5", False), ("lossless", True), ("abs5", False)])
def test_cells_equal_the_filtered_aggregate_per_cell(hip, eb_name, irregular):
    """(b): every cell against mdb_agg_batch_filter over the cell's bounds, with both time ranges set and overlapping
    partly."""
    batch, groups = _series_batch(cases.error_bounds()[eb_name], irregular, n_series=2, length=3000, seed=610)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    width = (last - first) // 9 + 1
    _, values, _, _ = _grid(batch)
    median = float(np.median(values))
    for flt in (mdb.value_filter(lo=median), mdb.value_filter(hi=median, hi_open=True, t_lo=first + width // 2),
                mdb.value_filter(lo=median - 10.0, hi=median + 10.0, t_lo=first + 3 * width + 17, t_hi=last - width)):
        for t_lo, t_hi in ((I64_MIN, I64_MAX), (first + 2 * width - 5, last - width // 3)):
            got = hip.agg_buckets_filter(batch, flt, first - 7, width, 11, groups=groups, t_lo=t_lo, t_hi=t_hi,
                                         n_groups=2)
            expected = _oracle_by_filtered_aggregates(hip, batch, groups, 2, first - 7, width, 11, flt, t_lo, t_hi)
            _assert_cells(got, expected, (eb_name, t_lo, t_hi))
            magnitudes = []
            _assert_cells(got, _oracle(batch, groups, 2, first - 7, width, 11, flt, t_lo, t_hi, magnitudes),
                          (eb_name, "grid"), magnitudes[0])


@pytest.mark.parametrize("eb_name", ["lossless", "abs5"])
def test_edge_cases_nan_inf_and_zeros(hip, eb_name):
    eb = cases.error_bounds()[eb_name]
    parts = [ora.try_compress_univariate_time_series(ts, v, eb) for _, ts, v in cases.edge_case_series()]
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    batch = mdb.SegmentBatch.concat(parts)
    nan, inf = float("nan"), float("inf")
    neg_nan = np.uint32(0xFFC00000).view(np.float32).item()
    specs = [dict(), dict(lo=0.0), dict(hi=-0.0), dict(lo=-0.0, hi=0.0), dict(lo=0.0, hi=0.0), dict(lo=-0.0, hi=-0.0),
             dict(lo=inf), dict(hi=-inf), dict(lo=nan), dict(hi=neg_nan), dict(lo=-inf, hi=inf),
             dict(lo=0.0, lo_open=True, hi=inf), dict(lo=-1e-45, hi=1e-45), dict(lo=37.0, hi=73.0, hi_open=True),
             dict(lo=3.0, hi=2.0), dict(lo=5.0, hi=5.0, hi_open=True), dict(lo=5.0, t_lo=150, t_hi=950),
             dict(hi=1e30, t_lo=-50, t_hi=1658671178037 + 4000)]
    for spec in specs:
        flt = mdb.value_filter(**spec)
        for origin, width, n_buckets in ((0, 100, 40), (-35, 250, 24), (1658671178037 - 1000, 3000, 30), (0, 1 << 40, 3)):
            _check(hip, batch, groups, len(parts), origin, width, n_buckets, flt, context=(eb_name, spec, width))


def test_swing_cut_by_a_bucket_edge_and_the_threshold_at_epoch_timestamps(hip):
    """Swing lines at 1.7e15 us (the rebuilt points can round past the stored extremes there) and crossing zero, bounds
    on every segment's stored min / max and their f32 neighbours, buckets shorter than the segments: within one segment
    a bucket edge and the threshold cut the model part."""
    eb = mdb.error_bound("absolute", 0.5)
    parts = []
    for k, slope in enumerate((1e-3, -1e-3, 2.5e-4, -7e-6)):
        ts = EPOCH_US + np.arange(3000, dtype=np.int64) * 1000 + k
        values = (slope * (np.arange(3000) - 1500.0 - 13.0 * k)).astype(np.float32)
        parts.append(ora.try_compress_univariate_time_series(ts, values, eb))
    batch = mdb.SegmentBatch.concat(parts)
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    swing = batch.model_type_id == mdb.MDB_SWING_ID
    assert swing.any() and (batch.end_time[swing] - batch.start_time[swing]).max() > 300_000
    specs = [dict(lo=0.0), dict(hi=-0.0), dict(lo=-0.0, hi=0.0), dict(lo=0.0, lo_open=True)]
    for i in np.nonzero(swing)[0][:12]:
        for v in (batch.min_value[i], batch.max_value[i]):
            for n in (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))):
                specs += [dict(lo=float(n)), dict(hi=float(n), hi_open=True)]
    for spec in specs:
        flt = mdb.value_filter(**spec)
        for origin, width in ((EPOCH_US - 333, 250_000), (EPOCH_US + 77_777, 1_000_003)):
            n_buckets = (3000 * 1000) // width + 2
            _check(hip, batch, groups, 4, origin, width, n_buckets, flt, context=(spec, width))


def _profiled(hip, call):
    hip.profile_enable(True)
    hip.profile_reset()
    try:
        result = call()
        return result, hip.profile()
    finally:
        hip.profile_enable(False)


def test_macaque_v_through_the_cursor_index_and_without(hip, monkeypatch):
    """Lossless MacaqueV streams of 65 536 values: piece by piece from the cursor index (resident batch, and the host
    forms) in k_agg_bucket_pieces_filter, and one lane per stream with MDB_GRID_MV_INDEX=0. Both match (a)."""
    n = 140_000
    rng = np.random.default_rng(47)
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
    _, values, _, _ = _grid(batch)
    threshold = float(np.quantile(values, 0.6))
    resident = hip.upload_segments(batch)
    try:
        for flt in (mdb.value_filter(lo=threshold), mdb.value_filter(hi=threshold, t_lo=3_000_000, t_hi=11_000_000)):
            for origin, width, n_buckets in ((0, 777 * INTERVAL, 190), (13, 3 * INTERVAL, 48_000)):
                args = (flt, origin, width, n_buckets)
                host, kernels = _profiled(hip, lambda: hip.agg_buckets_filter(batch, *args, groups=groups, n_groups=2))
                assert "k_agg_bucket_pieces_filter" in kernels and "k_agg_bucket_pieces" not in kernels, kernels
                assert "k_agg_bucket_partials_filter" in kernels and "k_agg_bucket_partials" not in kernels, kernels
                magnitudes = []
                expected = _oracle(batch, groups, 2, origin, width, n_buckets, flt, magnitudes=magnitudes)
                _assert_cells(host, expected, ("index", width), magnitudes[0])
                on_device = hip.agg_buckets_filter_dev(resident, *args, groups=groups, n_groups=2)
                assert on_device.tobytes() == host.tobytes()
                monkeypatch.setenv("MDB_GRID_MV_INDEX", "0")
                try:
                    plain, kernels = _profiled(hip, lambda: hip.agg_buckets_filter(batch, *args, groups=groups,
                                                                                   n_groups=2))
                    assert "k_agg_bucket_pieces_filter" not in kernels, kernels
                    _assert_cells(plain, expected, ("no index", width), magnitudes[0])
                    unindexed = hip.agg_buckets_filter_dev(resident, *args, groups=groups, n_groups=2)
                    _assert_cells(unindexed, expected, ("no index, resident", width), magnitudes[0])
                finally:
                    monkeypatch.delenv("MDB_GRID_MV_INDEX")
    finally:
        resident.free()


def test_determinism_across_runs_forms_slices_and_orders(hip, monkeypatch):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, n_series=4, length=20_000, seed=420)
    lossless, lossless_groups = _series_batch(cases.LOSSLESS, True, n_series=2, length=8_000, seed=430)
    batch = mdb.SegmentBatch.concat([batch, lossless])
    groups = np.concatenate([groups, lossless_groups + 4])
    _, values, _, _ = _grid(batch)
    flt = mdb.value_filter(lo=float(np.quantile(values, 0.3)), t_lo=int(batch.start_time.min()) + 123_456)
    args = (flt, -777, 1_300, 1_600)
    request_range = dict(t_lo=50_000, t_hi=int(batch.end_time.max()) - 77_777)
    first = hip.agg_buckets_filter(batch, *args, groups=groups, n_groups=6, **request_range)
    second = hip.agg_buckets_filter(batch, *args, groups=groups, n_groups=6, **request_range)
    assert first.tobytes() == second.tobytes()
    cut = [0, len(batch) // 3, 2 * len(batch) // 3, len(batch)]
    listed = hip.agg_buckets_filter_list([batch.slice(cut[k], cut[k + 1]) for k in range(3)], *args,
                                         groups=[groups[cut[k]:cut[k + 1]] for k in range(3)], n_groups=6,
                                         **request_range)
    assert listed.tobytes() == first.tobytes()
    resident = hip.upload_segments(batch)
    on_device = hip.agg_buckets_filter_dev(resident, *args, groups=groups, n_groups=6, **request_range)
    assert on_device.tobytes() == first.tobytes()
    resident.free()
    magnitudes = []
    expected = _oracle(batch, groups, 6, -777, 1_300, 1_600, flt, magnitudes=magnitudes, **request_range)
    _assert_cells(first, expected, "default", magnitudes[0])
    monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "1000")
    sliced = hip.agg_buckets_filter(batch, *args, groups=groups, n_groups=6, **request_range)
    _assert_cells(sliced, expected, "slices of 1000 pairs", magnitudes[0])
    monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
    order = np.random.default_rng(5).permutation(len(batch))
    shuffled = batch.take(order)
    got = hip.agg_buckets_filter(shuffled, *args, groups=groups[order], n_groups=6, **request_range)
    _assert_cells(got, expected, "shuffled (sort path)", magnitudes[0])
    again = hip.agg_buckets_filter(shuffled, *args, groups=groups[order], n_groups=6, **request_range)
    assert again.tobytes() == got.tobytes()


def test_an_all_pass_filter_is_bit_identical_to_agg_buckets(hip):
    """No value bounds over the whole time range: the same pairs, entries, tree and closed forms as mdb_agg_buckets -
    the same bits, for every form. A filter's time range gives the bits of the request narrowed to it."""
    for eb_name, irregular in (("rel5", False), ("abs5", True), ("lossless", False), ("lossless", True)):
        batch, groups = _series_batch(cases.error_bounds()[eb_name], irregular, n_series=3, length=8000, seed=650)
        _, values, _, _ = _grid(batch)
        assert np.isfinite(values).all()
        first, last = int(batch.start_time.min()), int(batch.end_time.max())
        every = mdb.value_filter()
        for origin, width, n_buckets in ((first, 700, (last - first) // 700 + 1), (first - 5, 100_000, 9)):
            plain = hip.agg_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=3)
            filtered = hip.agg_buckets_filter(batch, every, origin, width, n_buckets, groups=groups, n_groups=3)
            assert filtered.tobytes() == plain.tobytes(), (eb_name, width)
            resident = hip.upload_segments(batch)
            try:
                on_device = hip.agg_buckets_filter_dev(resident, every, origin, width, n_buckets, groups=groups,
                                                       n_groups=3)
                assert on_device.tobytes() == hip.agg_buckets_dev(resident, origin, width, n_buckets, groups=groups,
                                                                  n_groups=3).tobytes()
            finally:
                resident.free()
            t_lo, t_hi = first + 12_345, last - 23_456
            ranged = hip.agg_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=3, t_lo=t_lo, t_hi=t_hi)
            timed = hip.agg_buckets_filter(batch, mdb.value_filter(t_lo=t_lo, t_hi=t_hi), origin, width, n_buckets,
                                           groups=groups, n_groups=3)
            assert timed.tobytes() == ranged.tobytes(), (eb_name, width, "time range")


def test_one_bucket_equals_the_filtered_aggregate(hip):
    for eb_name, irregular in (("lossless", False), ("rel5", True), ("abs5", False)):
        batch, groups = _series_batch(cases.error_bounds()[eb_name], irregular)
        first, last = int(batch.start_time.min()), int(batch.end_time.max())
        for _, flt in _predicates(batch):
            got = hip.agg_buckets_filter(batch, flt, first, last - first + 1, 1, groups=groups, n_groups=3)
            for g in range(3):
                state = hip.agg_filter(batch.take(np.nonzero(groups == g)[0]), flt, ALL)
                assert got[g, 0]["count"] == state.count
                assert np.float32(got[g, 0]["min"]).view(np.uint32) == np.float32(state.min).view(np.uint32)
                assert np.float32(got[g, 0]["max"]).view(np.uint32) == np.float32(state.max).view(np.uint32)
                assert abs(got[g, 0]["sum"] - state.sum) <= SUM_TOLERANCE * abs(state.sum)


def test_cells_without_a_passing_point_stay_as_they_were(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, length=4000, seed=660)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    _, values, _, _ = _grid(batch)
    flt = mdb.value_filter(lo=float(np.quantile(values, 0.9)))
    n_buckets = (last - first) // 1000 + 1
    rng = np.random.default_rng(661)
    prefilled = mdb.fresh_agg_states((3, n_buckets))
    prefilled["sum"] = rng.normal(size=(3, n_buckets)) * 100.0
    prefilled["count"] = rng.integers(1, 100, size=(3, n_buckets))
    prefilled["min"] = rng.uniform(90.0, 150.0, size=(3, n_buckets)).astype(np.float32)
    prefilled["max"] = rng.uniform(150.0, 250.0, size=(3, n_buckets)).astype(np.float32)
    expected = _oracle(batch, groups, 3, first, 1000, n_buckets, flt)
    hit = expected["count"] > 0
    assert hit.any() and (~hit).any()
    for form in ("host", "dev"):
        states = prefilled.copy()
        if form == "host":
            hip.agg_buckets_filter(batch, flt, first, 1000, n_buckets, groups=groups, states=states)
        else:
            resident = hip.upload_segments(batch)
            try:
                hip.agg_buckets_filter_dev(resident, flt, first, 1000, n_buckets, groups=groups, states=states)
            finally:
                resident.free()
        assert states[~hit].tobytes() == prefilled[~hit].tobytes(), form
        np.testing.assert_array_equal(states["count"][hit], prefilled["count"][hit] + expected["count"][hit])
        np.testing.assert_array_equal(states["min"][hit], np.fmin(prefilled["min"][hit], expected["min"][hit]))
        np.testing.assert_array_equal(states["max"][hit], np.fmax(prefilled["max"][hit], expected["max"][hit]))
        total = prefilled["sum"][hit] + expected["sum"][hit]
        assert np.all(np.abs(states["sum"][hit] - total) <= SUM_TOLERANCE * np.abs(expected["sum"][hit]) + 1e-9), form


def test_errors_leave_the_cells_untouched(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, length=2000, seed=670)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    rng = np.random.default_rng(9)
    states = mdb.fresh_agg_states((3, 10))
    states["sum"] = rng.normal(size=(3, 10))
    states["count"] = rng.integers(0, 100, size=(3, 10))
    before = states.copy()
    good = mdb.value_filter(lo=150.0)
    bad_flags = mdb.value_filter(lo=150.0)
    bad_flags.flags |= 16
    bad_reserved = mdb.value_filter(lo=150.0)
    bad_reserved.reserved = 1
    resident = hip.upload_segments(batch)
    lib, handle = hip.lib, hip.handle
    cells = states.ctypes.data_as(C.c_void_p)
    request = _abi.BucketRequestC(first, 1000, 10, I64_MIN, I64_MAX, 3, ALL)
    seg = batch.as_c()
    inputs = (C.POINTER(_abi.SegmentsC) * 1)(C.pointer(seg))
    group_pointers = (C.c_void_p * 1)(None)
    try:
        # NULL arguments (one at a time)
        for host_seg, dev_seg in ((C.byref(seg), C.byref(resident.seg)), (None, None)):
            for args in ((C.byref(request), C.byref(good), cells) if host_seg is None else
                         (None, C.byref(good), cells), (C.byref(request), None, cells), (C.byref(request), C.byref(good), None)):
                assert lib.mdb_agg_buckets_filter(handle, host_seg, None, *args) != 0
                assert lib.mdb_agg_buckets_filter_dev(handle, dev_seg, None, *args) != 0
        assert lib.mdb_agg_buckets_filter_list(handle, None, group_pointers, 1, C.byref(request), C.byref(good),
                                               cells) != 0
        assert lib.mdb_agg_buckets_filter_list(handle, inputs, group_pointers, 1, C.byref(request), None, cells) != 0
        null_input = (C.POINTER(_abi.SegmentsC) * 1)()
        assert lib.mdb_agg_buckets_filter_list(handle, null_input, group_pointers, 1, C.byref(request), C.byref(good),
                                               cells) != 0
        assert states.tobytes() == before.tobytes()
        # the filter's flags and reserved field; the request's width, n_groups and cell count
        for bad in (bad_flags, bad_reserved):
            for call in (lambda: hip.agg_buckets_filter(batch, bad, first, 1000, 10, groups=groups, states=states),
                         lambda: hip.agg_buckets_filter_list([batch], bad, first, 1000, 10, groups=[groups],
                                                             states=states),
                         lambda: hip.agg_buckets_filter_dev(resident, bad, first, 1000, 10, groups=groups,
                                                            states=states)):
                with pytest.raises(mdb.HipError):
                    call()
                assert states.tobytes() == before.tobytes()
        for width, n_groups, n_buckets in ((0, 3, 10), (-100, 3, 10), (1000, 0, 10), (1000, 2, 1 << 63)):
            bad_request = _abi.BucketRequestC(first, width, n_buckets, I64_MIN, I64_MAX, n_groups, ALL)
            assert lib.mdb_agg_buckets_filter(handle, C.byref(seg), None, C.byref(bad_request), C.byref(good),
                                              cells) != 0
            assert lib.mdb_agg_buckets_filter_dev(handle, C.byref(resident.seg), None, C.byref(bad_request),
                                                  C.byref(good), cells) != 0
        assert states.tobytes() == before.tobytes()
        # a group id >= n_groups: reported with any predicate, an empty value interval and an empty time intersection
        bad = groups.copy()
        bad[len(bad) // 2] = 3
        nothing = mdb.value_filter(lo=5.0, hi=5.0, hi_open=True)
        apart = mdb.value_filter(lo=150.0, t_lo=last + 10, t_hi=last + 20)
        for flt, t_lo, t_hi in ((good, None, None), (nothing, None, None), (apart, first, last)):
            for call in (lambda: hip.agg_buckets_filter(batch, flt, first, 1000, 10, groups=bad, states=states,
                                                        t_lo=t_lo, t_hi=t_hi),
                         lambda: hip.agg_buckets_filter_list([batch.slice(0, 5), batch.slice(5, len(batch))], flt,
                                                             first, 1000, 10, groups=[bad[:5], bad[5:]],
                                                             states=states, t_lo=t_lo, t_hi=t_hi)):
                with pytest.raises(mdb.HipError):
                    call()
                assert states.tobytes() == before.tobytes()
            # the dev form on device cells, read back after the error
            dev_groups, dev_cells = hip.upload_array(bad), hip.upload_array(states)
            try:
                bad_request = hip._bucket_request(first, 1000, 10, 3, t_lo, t_hi, ALL)
                assert lib.mdb_agg_buckets_filter_dev(handle, C.byref(resident.seg), C.c_void_p(dev_groups),
                                                      C.byref(bad_request), C.byref(flt), C.c_void_p(dev_cells)) != 0
                assert hip.download_array(dev_cells, states.size, mdb.AGG_STATE_DTYPE).tobytes() == before.tobytes()
            finally:
                hip.dev_free(dev_groups)
                hip.dev_free(dev_cells)
        # ... and without the bad id they select nothing, and succeed
        for flt, t_lo, t_hi in ((nothing, None, None), (apart, first, last)):
            hip.agg_buckets_filter(batch, flt, first, 1000, 10, groups=groups, states=states, t_lo=t_lo, t_hi=t_hi)
            assert states.tobytes() == before.tobytes()
    finally:
        resident.free()


def test_fuzzed_segments_filters_and_requests(hip):
    """Segments of the edge-case and mixed batches, some with a field changed or a payload cut or flipped, under random
    predicates and requests: an error exactly where mdb_agg_buckets (its range narrowed to the filter's) reports one,
    and otherwise cells that agree with (a)."""
    rng = np.random.default_rng(2027)
    pool = []
    for eb_name in ("lossless", "rel5"):
        pool += cases.edge_case_batch(cases.error_bounds()[eb_name]).rows()
        for irregular in (False, True):
            pool += cases.mixed_batch(cases.error_bounds()[eb_name], irregular, seed=733, length=3000)[2].rows()
    agree = errors = 0
    for trial in range(160):
        rows = []
        for _ in range(int(rng.integers(1, 6))):
            row = list(pool[int(rng.integers(0, len(pool)))])
            if rng.random() < 0.35:
                field = int(rng.choice([0, 1, 2, 3, 6, 7]))
                if field == 0:
                    row[0] = int(rng.integers(0, 4))
                elif field in (1, 2):
                    row[field] = int(row[field] + rng.integers(-500, 500))
                else:
                    payload = bytearray(row[field])
                    action = rng.integers(0, 3)
                    if action == 0 and payload:
                        payload = payload[: int(rng.integers(0, len(payload)))]
                    elif action == 1 and payload:
                        payload[int(rng.integers(0, len(payload)))] ^= 1 << int(rng.integers(0, 8))
                    else:
                        payload = bytearray(rng.integers(0, 256, size=int(rng.integers(0, 20)), dtype=np.uint8).tobytes())
                    row[field] = bytes(payload)
            rows.append(tuple(row))
        batch = mdb.SegmentBatch.from_rows(rows)
        first, last = int(batch.start_time.min()), int(batch.end_time.max())
        origin, width, n_buckets = first - int(rng.integers(0, 1000)), int(rng.integers(50, 5000)), 6
        t_lo, t_hi = I64_MIN, I64_MAX
        if rng.random() < 0.3:
            t_lo = first + int(rng.integers(0, 3000))
        lo = float(rng.uniform(-50.0, 250.0)) if rng.integers(3) else None
        hi = float(rng.uniform(-50.0, 250.0)) if rng.integers(3) else None
        spec = dict(lo=lo, hi=hi, lo_open=bool(rng.integers(2)), hi_open=bool(rng.integers(2)))
        if rng.random() < 0.4:
            spec.update(t_lo=first + int(rng.integers(-100, 4000)), t_hi=last - int(rng.integers(-100, 4000)))
        flt = mdb.value_filter(**spec)
        try:
            if ora.agg_batch(batch, ALL).count > 200_000:
                continue
            ora.grid_batch(batch)
            magnitudes = []
            expected = _oracle(batch, None, 1, origin, width, n_buckets, flt, t_lo, t_hi, magnitudes)
        except ora.OracleError:
            expected = None
        try:
            got = hip.agg_buckets_filter(batch, flt, origin, width, n_buckets, t_lo=t_lo, t_hi=t_hi)
        except mdb.HipError:
            got = None
        try:
            hip.agg_buckets(batch, origin, width, n_buckets, t_lo=max(t_lo, flt.t_lo), t_hi=min(t_hi, flt.t_hi))
            plain_failed = False
        except mdb.HipError:
            plain_failed = True
        assert (got is None) == plain_failed, (trial, rows, spec)
        if expected is not None:
            assert got is not None, (trial, rows)
            _assert_cells(got, expected, (trial, spec), magnitudes[0])
            agree += 1
        else:
            errors += got is None
    assert agree > 30 and errors > 10, (agree, errors)
