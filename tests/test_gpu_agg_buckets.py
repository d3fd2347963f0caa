"""COUNT / MIN / MAX / SUM per date_bin bucket and group (mdb_agg_buckets*) against the reference's fallback plan:
GridExec -> date_bin / range filter -> GROUP BY, restated by the oracle as ora.agg_batch_range over each bucket's
bounds (small cases) or as numpy bucketing of ora.grid_batch's points (large ones). COUNT / MIN / MAX exact, SUM
within 0.001 %."""

import numpy as np
import pytest

import cases
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM

pytestmark = pytest.mark.gpu

ALL = MDB_AGG_COUNT | MDB_AGG_MIN | MDB_AGG_MAX | MDB_AGG_SUM
SUM_TOLERANCE = 1e-5
INTERVAL = 100  # the sampling interval of tests/datagen.py
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _series_batch(eb, irregular, n_series=3, length=6000, seed=400):
    parts = [cases.mixed_batch(eb, irregular, seed=seed + k, length=length)[2] for k in range(n_series)]
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    return mdb.SegmentBatch.concat(parts), groups


def _oracle_by_ranges(batch, groups, n_groups, origin, width, n_buckets, t_lo=I64_MIN, t_hi=I64_MAX):
    """Cell (g, b): ora.agg_batch_range on the segments of group g over the bucket's bounds AND [t_lo, t_hi]."""
    out = mdb.fresh_agg_states((n_groups, n_buckets))
    groups = np.zeros(len(batch), dtype=np.uint32) if groups is None else groups
    for g in range(n_groups):
        rows = np.nonzero(groups == g)[0]
        if len(rows) == 0:
            continue
        part = batch.take(rows)
        for b in range(n_buckets):
            lo, hi = max(origin + b * width, t_lo), min(origin + (b + 1) * width - 1, t_hi, I64_MAX)
            if lo > hi:
                continue
            state = ora.agg_batch_range(part, lo, hi, ALL)
            if state.count:
                out[g, b] = (state.sum, state.count, state.min, state.max)
    return out


def _oracle_by_grid(batch, groups, n_groups, origin, width, n_buckets, t_lo=I64_MIN, t_hi=I64_MAX, magnitudes=None):
    """The points of ora.grid_batch, bucketed with numpy (date_bin's floor, Python integers for the bounds).
    `magnitudes` (a list): receives the sum of |value| per cell."""
    timestamps, values, rows, _ = ora.grid_batch(batch)
    groups = np.zeros(len(batch), dtype=np.uint32) if groups is None else groups
    point_groups = np.repeat(groups.astype(np.int64), rows.astype(np.int64))
    keep = (timestamps >= t_lo) & (timestamps <= t_hi)
    diff = timestamps.astype(object) - origin
    buckets = np.array([d // width for d in diff], dtype=object) if len(diff) else np.zeros(0, dtype=object)
    keep &= np.array([0 <= b < n_buckets for b in buckets], dtype=bool) if len(buckets) else np.zeros(0, dtype=bool)
    keys = point_groups[keep] * n_buckets + buckets[keep].astype(np.int64)
    picked = values[keep].astype(np.float32)
    out = mdb.fresh_agg_states(n_groups * n_buckets)
    counts = np.bincount(keys, minlength=n_groups * n_buckets)
    sums = np.zeros(n_groups * n_buckets)
    np.add.at(sums, keys, picked.astype(np.float64))
    mins = np.full(n_groups * n_buckets, np.float32(ora_f32_max()), dtype=np.float32)
    maxs = np.full(n_groups * n_buckets, -np.float32(ora_f32_max()), dtype=np.float32)
    np.fmin.at(mins, keys, picked)
    np.fmax.at(maxs, keys, picked)
    if magnitudes is not None:
        magnitude = np.zeros(n_groups * n_buckets)
        np.add.at(magnitude, keys, np.abs(picked.astype(np.float64)))
        magnitudes.append(magnitude.reshape(n_groups, n_buckets))
    hit = counts > 0
    out["count"][hit], out["sum"][hit], out["min"][hit], out["max"][hit] = counts[hit], sums[hit], mins[hit], maxs[hit]
    return out.reshape(n_groups, n_buckets)


def ora_f32_max():
    return np.finfo(np.float32).max


def _assert_cells(got, expected, context="", magnitude=None):
    """`magnitude` (sum of |value| per cell): for cells whose segments' sums cancel - the closed forms of Swing are held
    to 1e-6 of each segment's part (segment_range), not of the cell's total."""
    assert got.shape == expected.shape
    np.testing.assert_array_equal(got["count"], expected["count"], err_msg=context)
    np.testing.assert_array_equal(got["min"].view(np.uint32), expected["min"].view(np.uint32), err_msg=context)
    np.testing.assert_array_equal(got["max"].view(np.uint32), expected["max"].view(np.uint32), err_msg=context)
    finite = np.isfinite(expected["sum"])
    assert np.array_equal(got["sum"][~finite], expected["sum"][~finite], equal_nan=True), context
    diff = np.abs(got["sum"][finite] - expected["sum"][finite])
    bound = SUM_TOLERANCE * np.abs(expected["sum"][finite])   # (no absolute floor: cells of tiny values are held too)
    if magnitude is not None:
        bound = bound + 1e-6 * magnitude[finite]
    assert np.all(diff <= bound), (context, float(np.max(diff - bound)))


def _bucket_sets(first, last):
    """(name, origin, width, n_buckets, t_lo, t_hi) over data in [first, last]."""
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
def test_parity_with_the_fallback_plan(hip, eb_name, irregular):
    batch, groups = _series_batch(cases.error_bounds()[eb_name], irregular)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    for name, origin, width, n_buckets, t_lo, t_hi in _bucket_sets(first, last):
        got = hip.agg_buckets(batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=3)
        expected = _oracle_by_grid(batch, groups, 3, origin, width, n_buckets, t_lo, t_hi)
        _assert_cells(got, expected, f"{eb_name} {name}")
        if n_buckets <= 40:  # the range oracle cell by cell as well
            _assert_cells(got, _oracle_by_ranges(batch, groups, 3, origin, width, n_buckets, t_lo, t_hi), name)


@pytest.mark.parametrize("eb_name", ["lossless", "rel5"])
def test_edge_case_series(hip, eb_name):
    """NaN, infinities, one- and two-point segments, long residual tails, huge timestamp gaps: every edge case of the
    suite as its own group, bucketed at several widths against the range oracle."""
    eb = cases.error_bounds()[eb_name]
    parts = [ora.try_compress_univariate_time_series(ts, v, eb) for _, ts, v in cases.edge_case_series()]
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    batch = mdb.SegmentBatch.concat(parts)
    for origin, width, n_buckets in ((0, 100, 40), (-35, 250, 24), (1658671178037 - 1000, 3000, 30), (0, 1 << 40, 3)):
        got = hip.agg_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=len(parts))
        # (|value| per cell: a tail of -FLT_MAX, +FLT_MAX behind a model adding up to 468 is 0 in the oracle's sequential
        # f64 sum and 468 when the tail is added up on its own)
        magnitudes = []
        _oracle_by_grid(batch, groups, len(parts), origin, width, n_buckets, magnitudes=magnitudes)
        _assert_cells(got, _oracle_by_ranges(batch, groups, len(parts), origin, width, n_buckets),
                      f"{eb_name} {origin} {width}", magnitudes[0])


def test_negative_timestamps_floor(hip):
    """Points before the origin and at negative times: b = floor((ts - origin) / width), not truncation."""
    timestamps = np.arange(-5000, 5000, 100, dtype=np.int64)
    values = (np.sin(np.arange(len(timestamps)) / 7.0) * 50).astype(np.float32)
    for eb in (cases.LOSSLESS, mdb.error_bound("absolute", 5.0)):
        batch = ora.try_compress_univariate_time_series(timestamps, values, eb)
        for origin, width, n_buckets in ((-4950, 300, 40), (-10_000, 1_000, 20), (7, 450, 30), (-3001, 1, 2500)):
            got = hip.agg_buckets(batch, origin, width, n_buckets)
            _assert_cells(got, _oracle_by_grid(batch, None, 1, origin, width, n_buckets), f"{origin} {width}")


def test_extreme_origin_and_width_do_not_overflow(hip):
    timestamps = np.array([-(1 << 62), -5, 0, 17, 1 << 40, (1 << 62) + 3], dtype=np.int64)
    values = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], dtype=np.float32)
    batch = ora.try_compress_univariate_time_series(timestamps, values, cases.LOSSLESS)
    for origin, width, n_buckets, t_lo, t_hi in ((I64_MIN, (1 << 62) - 1, 8, I64_MIN, I64_MAX),
                                                 (I64_MIN + 1, 1 << 62, 4, I64_MIN, I64_MAX),
                                                 (I64_MIN, I64_MAX, 2, I64_MIN, I64_MAX),
                                                 (I64_MAX - 10, 1 << 62, 3, I64_MIN, I64_MAX),
                                                 (-(1 << 62), 1 << 61, 5, -100, I64_MAX)):
        got = hip.agg_buckets(batch, origin, width, n_buckets, t_lo=t_lo, t_hi=t_hi)
        _assert_cells(got, _oracle_by_ranges(batch, None, 1, origin, width, n_buckets, t_lo, t_hi), f"{origin} {width}")


def test_no_buckets_and_bad_requests_leave_the_cells_alone(hip):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, length=2000)
    rng = np.random.default_rng(9)
    states = mdb.fresh_agg_states((3, 10))
    states["sum"] = rng.normal(size=(3, 10))
    states["count"] = rng.integers(0, 100, size=(3, 10))
    before = states.copy()
    empty = np.zeros((3, 0), dtype=mdb.AGG_STATE_DTYPE)
    hip.agg_buckets(batch, 0, 100, 0, groups=groups, states=empty)
    for kwargs in (dict(width=0), dict(width=-100)):
        with pytest.raises(mdb.HipError):
            hip.agg_buckets(batch, 0, kwargs["width"], 10, groups=groups, states=states)
        assert states.tobytes() == before.tobytes()
    with pytest.raises(mdb.HipError):
        hip.agg_buckets(batch, 0, 100, 10, groups=groups, states=np.zeros((0, 10), dtype=mdb.AGG_STATE_DTYPE))
    bad = groups.copy()
    bad[len(bad) // 2] = 3
    for call in (lambda: hip.agg_buckets(batch, 0, 1000, 10, groups=bad, states=states),
                 lambda: hip.agg_buckets_list([batch.slice(0, 5), batch.slice(5, len(batch))], 0, 1000, 10,
                                              groups=[bad[:5], bad[5:]], states=states)):
        with pytest.raises(mdb.HipError):
            call()
        assert states.tobytes() == before.tobytes()
    resident = hip.upload_segments(batch)
    with pytest.raises(mdb.HipError):
        hip.agg_buckets_dev(resident, 0, 1000, 10, groups=bad, states=states)
    assert states.tobytes() == before.tobytes()
    resident.free()


def test_long_macaque_v_streams_cut_in_their_middle(hip):
    """Lossless MacaqueV streams of 65 536 values (200 k points per series in chunks of 65 536, regular and irregular
    timestamps) with buckets that cut the streams in their middle."""
    import datagen
    n = 200_000
    rng = np.random.default_rng(41)
    regular = np.arange(n, dtype=np.int64) * INTERVAL
    irregular = np.concatenate([[0], np.cumsum(rng.integers(50, 150, n - 1))]).astype(np.int64)
    parts = []
    for k, timestamps in enumerate((regular, irregular)):
        values = datagen.sine_series(11 + k, n)[1]
        offsets = np.append(np.arange(0, n, 65536), n).astype(np.uint64)
        parts.append(hip.compress_chunks(timestamps, values, offsets, cases.LOSSLESS))
    batch = mdb.SegmentBatch.concat(parts)
    assert int((batch.model_type_id == 2).sum()) >= 6
    groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(parts)])
    for origin, width, n_buckets in ((0, 777 * INTERVAL, 260), (-55, 40_000 * INTERVAL + 3, 6), (13, 3 * INTERVAL, 66_700)):
        got = hip.agg_buckets(batch, origin, width, n_buckets, groups=groups, n_groups=2)
        _assert_cells(got, _oracle_by_grid(batch, groups, 2, origin, width, n_buckets), f"{width}")


def test_one_bucket_equals_the_range_aggregate_and_halves_add_up(hip):
    for eb_name, irregular in (("lossless", False), ("rel5", True), ("abs5", False)):
        batch, groups = _series_batch(cases.error_bounds()[eb_name], irregular)
        t_lo, t_hi = 12_345, 401_234
        got = hip.agg_buckets(batch, t_lo, t_hi - t_lo + 1, 1, groups=groups, n_groups=3)
        for g in range(3):
            state = hip.agg_batch_range(batch.take(np.nonzero(groups == g)[0]), t_lo, t_hi, ALL)
            expected = np.array([(state.sum, state.count, state.min, state.max)], dtype=mdb.AGG_STATE_DTYPE)
            _assert_cells(got[g:g + 1], expected.reshape(1, 1), f"{eb_name} group {g}")
        whole = hip.agg_buckets(batch, 0, 3_000, 200, groups=groups, n_groups=3)
        half = len(batch) // 2
        halves = hip.agg_buckets(batch.slice(0, half), 0, 3_000, 200, groups=groups[:half], n_groups=3)
        halves = hip.agg_buckets(batch.slice(half, len(batch)), 0, 3_000, 200, groups=groups[half:], states=halves)
        _assert_cells(halves, whole, eb_name)


def test_determinism_across_runs_forms_slices_and_orders(hip, monkeypatch):
    batch, groups = _series_batch(cases.error_bounds()["rel5"], False, n_series=4, length=20_000, seed=420)
    lossless, lossless_groups = _series_batch(cases.LOSSLESS, True, n_series=2, length=8_000, seed=430)
    batch = mdb.SegmentBatch.concat([batch, lossless])
    groups = np.concatenate([groups, lossless_groups + 4])
    args = (-777, 1_300, 1_600)
    first = hip.agg_buckets(batch, *args, groups=groups, n_groups=6)
    second = hip.agg_buckets(batch, *args, groups=groups, n_groups=6)
    assert first.tobytes() == second.tobytes()
    cut = [0, len(batch) // 3, 2 * len(batch) // 3, len(batch)]
    listed = hip.agg_buckets_list([batch.slice(cut[k], cut[k + 1]) for k in range(3)], *args,
                                  groups=[groups[cut[k]:cut[k + 1]] for k in range(3)], n_groups=6)
    assert listed.tobytes() == first.tobytes()
    resident = hip.upload_segments(batch)
    on_device = hip.agg_buckets_dev(resident, *args, groups=groups, n_groups=6)
    assert on_device.tobytes() == first.tobytes()
    resident.free()
    expected = _oracle_by_grid(batch, groups, 6, *args)
    _assert_cells(first, expected, "default")
    monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "1000")
    sliced = hip.agg_buckets(batch, *args, groups=groups, n_groups=6)
    _assert_cells(sliced, expected, "slices of 1000 pairs")
    monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
    order = np.random.default_rng(5).permutation(len(batch))
    shuffled = batch.take(order)
    got = hip.agg_buckets(shuffled, *args, groups=groups[order], n_groups=6)
    _assert_cells(got, expected, "shuffled (sort path)")
    assert hip.agg_buckets(shuffled, *args, groups=groups[order], n_groups=6).tobytes() == got.tobytes()
    # one group over all series: keys out of order across series, the sort path too
    everything = hip.agg_buckets(batch, *args)
    magnitudes = []
    expected_one = _oracle_by_grid(batch, None, 1, *args, magnitudes=magnitudes)
    _assert_cells(everything, expected_one, "one group", magnitudes[0])


def test_runs_of_one_cell_through_every_level_of_the_reduction_tree(hip):
    """More than 4 096 pairs in one cell: the fold walks the 64-entry tiles of level 0, then levels 1 and 2 - in pair
    order (one bucket: every key the same) and on the sort path (two buckets over copies of one series: keys 0, 1, 0,
    1, ... until sorted)."""
    base, _ = _series_batch(cases.error_bounds()["rel5"], False, n_series=1, length=6000, seed=440)
    big = base.take(np.tile(np.arange(len(base)), 5000 // len(base) + 2))
    assert len(big) > 4096
    first, last = int(big.start_time.min()), int(big.end_time.max())
    for width, n_buckets in ((last - first + 1, 1), ((last - first) // 2 + 1, 2)):
        got = hip.agg_buckets(big, first, width, n_buckets)
        magnitudes = []
        expected = _oracle_by_grid(big, None, 1, first, width, n_buckets, magnitudes=magnitudes)
        _assert_cells(got, expected, f"{n_buckets} bucket(s)", magnitudes[0])
        resident = hip.upload_segments(big)
        assert hip.agg_buckets_dev(resident, first, width, n_buckets).tobytes() == got.tobytes()
        resident.free()


def test_fuzzed_segments_never_hang_and_agree_with_the_oracle(hip):
    """The generator of test_gpu_agg.py's fuzz test: an error or a result that agrees with the oracle."""
    rng = np.random.default_rng(531)
    pool = []
    for eb_name in ("lossless", "rel5"):
        pool += cases.edge_case_batch(cases.error_bounds()[eb_name]).rows()
        for irregular in (False, True):
            pool += cases.mixed_batch(cases.error_bounds()[eb_name], irregular, seed=532, length=3000)[2].rows()
    agree = errors = 0
    for trial in range(200):
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
        first = int(batch.start_time.min())
        origin, width, n_buckets = first - int(rng.integers(0, 1000)), int(rng.integers(50, 5000)), 6
        try:
            if ora.agg_batch(batch, ALL).count > 200_000:
                continue
            ora.grid_batch(batch)
            expected = _oracle_by_ranges(batch, None, 1, origin, width, n_buckets)
            # (|value| per cell: +-3.4e38 beside small values cancel differently in another order of additions)
            magnitudes = []
            _oracle_by_grid(batch, None, 1, origin, width, n_buckets, magnitudes=magnitudes)
        except ora.OracleError:
            expected = None
        try:
            got = hip.agg_buckets(batch, origin, width, n_buckets)
        except mdb.HipError:
            got = None
        if expected is not None:
            assert got is not None, rows
            _assert_cells(got, expected, str(trial), magnitudes[0])
            agree += 1
        else:
            errors += got is None
    assert agree > 30 and errors > 10, (agree, errors)
