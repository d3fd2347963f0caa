"""The query operators (filtered grid and aggregates, per-bucket aggregates, row masks) at the sizes where their capped
launches loop, the scan takes its second level, the per-point segments need several default slices and row numbers
pass 2^32 (tests/scale_cases.py builds the three tiers; tests/test_query_scale_cpu.py checks its expected values).

Expected values never come from the library under test: the oracle's grid and numpy with the totalOrder key (tiers A
and B), closed forms for PMC-Mean and the oracle one segment at a time (tier C). Rows, values, rows_per_segment, masks,
COUNT, MIN and MAX bit for bit; SUM within 1e-5 of the sum of magnitudes.

Times and host peak: the "test suite" row of MEASUREMENTS.md; `pytest -s` prints them per tier."""

import resource
import time

import numpy as np
import pytest

import scale_cases as sc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import (MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM, MDB_MASK_AND, MDB_MASK_ANDNOT,
                              MDB_MASK_NOT, MDB_MASK_OR, MDB_MASK_XOR)

pytestmark = pytest.mark.gpu

ALL = MDB_AGG_COUNT | MDB_AGG_MIN | MDB_AGG_MAX | MDB_AGG_SUM
I64_MIN, I64_MAX = sc.I64_MIN, sc.I64_MAX
WORD_OPS = {MDB_MASK_AND: lambda a, b: a & b, MDB_MASK_OR: lambda a, b: a | b, MDB_MASK_XOR: lambda a, b: a ^ b,
            MDB_MASK_ANDNOT: lambda a, b: a & ~b}
_TIMES = {}  # seconds spent in library calls / building expected values, printed per tier (pytest -s)


class _Clock:
    def __init__(self, key):
        self.key = key

    def __enter__(self):
        self.started = time.perf_counter()

    def __exit__(self, *_):
        _TIMES[self.key] = _TIMES.get(self.key, 0.0) + time.perf_counter() - self.started


def _report(tier):
    peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6
    print(f"\n[scale] tier {tier}: library calls {_TIMES.get((tier, 'gpu'), 0.0):.1f} s, expected values "
          f"{_TIMES.get((tier, 'cpu'), 0.0):.1f} s, building {_TIMES.get((tier, 'build'), 0.0):.1f} s, "
          f"host peak so far {peak:.2f} GB")


class DeviceMask:
    """Device words for a mask over n_rows rows plus one guard word behind them, all pre-filled with 0xFF; compared
    packed (the mask is never unpacked)."""

    def __init__(self, context, n_rows):
        self.context, self.n_rows, self.words = context, n_rows, mdb.mask_words(n_rows)
        self.pointer = context.upload_array(np.full((self.words + 1) * 8, 0xFF, dtype=np.uint8))

    def check(self, expected_bytes, what):
        """The words are `expected_bytes` (whose padding bits are zero), the guard word is untouched."""
        raw = self.context.download_array(self.pointer, (self.words + 1) * 8, np.uint8)
        assert (raw[self.words * 8:] == 0xFF).all(), ("guard word", what)
        assert len(expected_bytes) == self.words * 8
        if self.n_rows % 64:  # (the expected padding really is zero)
            assert int(np.asarray(expected_bytes[-8:]).view(np.uint64)[0]) >> (self.n_rows % 64) == 0
        assert np.array_equal(raw[: self.words * 8], expected_bytes), what

    def free(self):
        self.context.dev_free(self.pointer)


def _profiled(hip, call):
    hip.profile_enable(True)
    hip.profile_reset()
    try:
        result = call()
        return result, hip.profile()
    finally:
        hip.profile_enable(False)


def _rows_by_type(batch, rows):
    return {name: int(rows[batch.model_type_id == k].sum()) for k, name in enumerate(mdb.MODEL_TYPE_NAMES)}


def _check_rows(got, field, picked, what):
    """(timestamps or None, values, rows_per_segment, metrics) against the rows `picked` (indices) of the field's grid."""
    ts, values, rows, metrics = got
    if ts is not None:
        assert np.array_equal(ts, field.ts[picked]), what
    assert np.array_equal(values.view(np.uint32), field.values[picked].view(np.uint32)), what
    expected_rows = np.bincount(field.segment[picked], minlength=len(field.batch)).astype(np.uint32)
    assert np.array_equal(rows, expected_rows), what
    assert metrics["rows_created"] == len(picked), what
    for name, count in _rows_by_type(field.batch, expected_rows).items():
        assert metrics[f"rows_created_by_{name}"] == count, (what, name)


def _upload(hip, fields):
    for field in fields:
        field.dev = hip.upload_segments(field.batch)


def _free(fields):
    for field in fields:
        if field.dev is not None:
            field.dev.free()
            field.dev = None


def _specs(field, few):
    """Bounds that pass about half, exactly one rebuilt value, a sliver at the low end, a band round the median."""
    median = float(np.median(field.values))
    picked = float(field.values[len(field.values) // 3])
    specs = [dict(lo=median), dict(lo=picked, hi=picked), dict(hi=float(np.percentile(field.values, 2)), hi_open=True),
             dict(lo=median - 3.0, hi=median + 3.0)]
    return specs[:2] if few else specs


def _check_operators(hip, tier, fields, ranges, few=False, n_buckets=1000, n_groups=4):
    """Every operator of the last four query features on fields[0] (the filters' field) and fields[1] (the target of
    the masks) under each time range and value filter."""
    a, b = fields
    cpu, gpu = _Clock((tier, "cpu")), _Clock((tier, "gpu"))
    rng = np.random.default_rng(9)
    groups = [rng.integers(0, n_groups, len(field.batch)).astype(np.uint32) for field in fields]
    first, last = int(a.ts.min()), int(a.ts.max())
    origin = first + (last - first) // 40  # (the first points lie in front of bucket 0, the last behind the last one)
    width = (last - first) // (n_buckets + 30)
    with cpu:
        specs = _specs(a, few)
        cells = [sc.Cells(field.ts, field.values, field.segment, group, n_groups, origin, width, n_buckets)
                 for field, group in zip(fields, groups)]
    for t_lo, t_hi in ranges:
        with cpu:
            inside = np.flatnonzero(a.in_range(t_lo, t_hi))
            in_range = np.zeros(len(a.ts), dtype=bool)
            in_range[inside] = True
            n_rows = len(inside)
        for f, field in enumerate(fields):
            with gpu:
                got = hip.agg_buckets_dev(field.dev, origin, width, n_buckets, groups=groups[f], t_lo=t_lo, t_hi=t_hi,
                                          n_groups=n_groups)
            with cpu:
                sc.check_cells(got, *cells[f].expected(in_range), (tier, "buckets", f, t_lo))
        mask_a, mask_b, out = (DeviceMask(hip, n_rows) for _ in range(3))
        try:
            with cpu:
                flt_b = mdb.value_filter(t_lo=t_lo, t_hi=t_hi, hi=float(np.median(b.values)))
                keep_b = sc.passes(b.keys[inside], flt_b)
                words_b = sc.pack_bits(keep_b)
            with gpu:
                assert hip.mask_filter_dev(b.dev, flt_b, mask_b.pointer, mask_b.words) == (n_rows, int(keep_b.sum()))
                mask_b.check(words_b, (tier, "mask b", t_lo))
            for s, spec in enumerate(specs):
                what = (tier, t_lo, spec)
                with cpu:
                    flt = mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **spec)
                    keep = sc.passes(a.keys[inside], flt)
                    picked, n_set = inside[keep], int(keep.sum())
                    words_a = sc.pack_bits(keep)
                    full = np.zeros(len(a.ts), dtype=bool)
                    full[picked] = True
                    expected_a, expected_b = sc.expected_agg(a.values[picked]), sc.expected_agg(b.values[picked])
                    expected_cells = cells[0].expected(full)
                # the filtered grid and aggregates of field a
                with gpu:
                    assert hip.grid_count_filter_dev(a.dev, flt) == n_set, what
                    rows = hip.grid_filter_resident(a.dev, flt)
                    state = hip.agg_filter_dev(a.dev, flt, ALL)
                    got_cells = hip.agg_buckets_filter_dev(a.dev, flt, origin, width, n_buckets, groups=groups[0],
                                                           n_groups=n_groups)
                with cpu:
                    _check_rows(rows, a, picked, what)
                    sc.check_agg(state, expected_a, what)
                    sc.check_cells(got_cells, *expected_cells, what)
                    del rows
                # the mask of the filter, and field b under it
                with gpu:
                    assert hip.mask_filter_dev(a.dev, flt, mask_a.pointer, mask_a.words) == (n_rows, n_set), what
                    mask_a.check(words_a, what)
                    rows = hip.grid_mask_resident(b.dev, t_lo, t_hi, mask_a.pointer, n_rows, n_set, values_only=(s % 2 == 1))
                    state = hip.agg_mask_dev(b.dev, t_lo, t_hi, mask_a.pointer, n_rows, ALL)
                with cpu:
                    assert (rows[0] is None) == (s % 2 == 1)
                    _check_rows(rows, b, picked, what)
                    sc.check_agg(state, expected_b, what)
                    del rows
                if s == 0:  # every op, out of place and in place; NOT clears the tail
                    for op, combine in WORD_OPS.items():
                        with cpu:
                            expected = combine(words_a.view(np.uint64), words_b.view(np.uint64)).view(np.uint8)
                            set_bits = int(combine(keep, keep_b).sum())
                        with gpu:
                            assert hip.mask_combine_dev(op, mask_a.pointer, mask_b.pointer, out.pointer, n_rows) == set_bits, (what, op)
                            out.check(expected, (what, op))
                    with gpu:
                        assert hip.mask_combine_dev(MDB_MASK_NOT, mask_a.pointer, None, out.pointer, n_rows) == n_rows - n_set
                        out.check(sc.pack_bits(~keep), (what, "not"))
                        assert hip.mask_combine_dev(MDB_MASK_AND, out.pointer, mask_b.pointer, out.pointer, n_rows) == int((~keep & keep_b).sum())
                        out.check(sc.pack_bits(~keep & keep_b), (what, "and in place"))
        finally:
            for mask in (mask_a, mask_b, out):
                mask.free()
    # the host forms once: two predicates over the two fields, the clipping range on one of them
    t_lo, t_hi = ranges[-1]
    with cpu:
        filters = [mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **specs[0]), mdb.value_filter(hi=float(np.median(b.values)))]
        inside = np.flatnonzero(a.in_range(t_lo, t_hi))
        picked = inside[sc.passes(a.keys[inside], filters[0]) & sc.passes(b.keys[inside], filters[1])]
    with gpu:
        state = hip.agg_where([a.batch, b.batch], filters, b.batch, ALL)
        rows = hip.grid_where([a.batch, b.batch], filters, b.batch)
    with cpu:
        sc.check_agg(state, sc.expected_agg(b.values[picked]), (tier, "agg_where"))
        _check_rows(rows, b, picked, (tier, "grid_where"))


def _clipping_range(field):
    """A range whose two ends fall between two points of one segment."""
    ts, segment = field.ts, field.segment
    k, j = len(ts) // 5, len(ts) - len(ts) // 3
    while segment[k] != segment[k + 1]:
        k += 1
    while segment[j - 1] != segment[j]:
        j += 1
    assert ts[k] + 1 < ts[j]
    return int(ts[k]) + 1, int(ts[j]) - 1


# ---- tier A: many segments ---------------------------------------------------------------------------------------------

def test_tier_a_many_segments(hip):
    with _Clock(("A", "build")):
        batches = sc.tier_a_batches(**sc.TIER_A)
        fields = [sc.Field(batch) for batch in batches]
    a, b = fields
    # the preconditions, from the batch and the oracle: past the scan's second level (1024 * 1024 segments), past the
    # caps of the wave-per-segment launches (65 536 segments) and of the word loops (524 288 words)
    assert len(a.batch) > 1_048_576 and len(b.batch) > 1_048_576 and len(a.batch) != len(b.batch)
    assert len(a.ts) > 33_554_432 and mdb.mask_words(len(a.ts)) > 524_288 and len(a.ts) % 64 != 0
    assert np.array_equal(a.ts, b.ts) and not np.array_equal(a.values.view(np.uint32), b.values.view(np.uint32))
    for field in fields:
        assert all(field.metrics[f"segments_with_{name}"] > 0 for name in mdb.MODEL_TYPE_NAMES), field.metrics
        assert field.metrics["segments_with_residuals"] > 0 and field.metrics["irregular_segments"] > 0
    assert sc.per_point_segments(a.batch).sum() > 2400  # (a few thousand)
    ranges = [(I64_MIN, I64_MAX), _clipping_range(a)]
    assert int(a.in_range(*ranges[1]).sum()) % 64 != 0
    _upload(hip, fields)
    try:
        _check_operators(hip, "A", fields, ranges)
    finally:
        _free(fields)
        hip.trim()
    _report("A")


# ---- tier B: default slices --------------------------------------------------------------------------------------------

def test_tier_b_default_slices(hip, monkeypatch):
    monkeypatch.delenv("MDB_FILTER_SLICE_POINTS", raising=False)
    with _Clock(("B", "build")):
        batches = sc.tier_b_batches(**sc.TIER_B)
        fields = [sc.Field(batch) for batch in batches]
    a, b = fields
    assert np.array_equal(a.ts, b.ts) and len(a.batch) != len(b.batch)
    for field in fields:  # more than three default slices of per-point rows, more than 32 768 segments in the first
        per_point = sc.per_point_segments(field.batch)
        rows = field.rows[per_point].astype(np.int64)
        assert int(rows.sum()) > 3 * (1 << 24) and int(per_point.sum()) >= 40_000
        assert int(np.searchsorted(np.cumsum(rows), 1 << 24, side="right")) > 32_768
    assert a.metrics["segments_with_residuals"] > 1000 and a.metrics["irregular_segments"] > 10_000
    whole, clipped = (I64_MIN, I64_MAX), _clipping_range(a)
    _upload(hip, fields)
    try:
        # the slicing happened: three launches at least of every kernel that works on a rebuilt slice
        flt = mdb.value_filter(lo=0.0)
        n_rows = len(a.ts)
        mask = DeviceMask(hip, n_rows)
        try:
            (_, n_set), kernels = _profiled(hip, lambda: hip.mask_filter_dev(a.dev, flt, mask.pointer, mask.words))
            assert kernels["k_mask_points_set"][0] >= 3, kernels
            _, kernels = _profiled(hip, lambda: hip.grid_mask_resident(b.dev, I64_MIN, I64_MAX, mask.pointer, n_rows, n_set))
            assert kernels["k_mask_points_write"][0] >= 3, kernels
            _, kernels = _profiled(hip, lambda: hip.grid_filter_resident(a.dev, flt))
            assert kernels["k_filter_points_count"][0] >= 3 and kernels["k_filter_points_write"][0] >= 3, kernels
        finally:
            mask.free()
        _check_operators(hip, "B", fields, [whole, clipped], few=True)
    finally:
        _free(fields)
        hip.trim()
    _report("B")


# ---- tier C: rows past 2^32 --------------------------------------------------------------------------------------------

N_GIANTS = sc.TIER_C["n_giants"]


@pytest.fixture(scope="module")
def tier_c(hip):
    with _Clock(("C", "build")):
        batches = sc.tier_c_batches(**sc.TIER_C)
        streams = [sc.Streamed(batch) for batch in batches]
    devs = [hip.upload_segments(batch) for batch in batches]
    yield streams, devs
    for dev in devs:
        dev.free()
    hip.trim()
    _report("C")


def _cells_of_one_group(hip, dev, flt, origin, width, n_buckets, t_lo=None, t_hi=None):
    if flt is None:
        return hip.agg_buckets_dev(dev, origin, width, n_buckets, t_lo=t_lo, t_hi=t_hi, n_groups=1)
    return hip.agg_buckets_filter_dev(dev, flt, origin, width, n_buckets, n_groups=1)


def _bucket_request(streamed, n_buckets=300):
    """Buckets whose edges cut the giants (a width that is no multiple of a giant's span), the first points in front of
    bucket 0 and the last behind the last one."""
    first, last = int(streamed.batch.start_time[0]), int(streamed.batch.end_time[-1])
    return first + 1_234_567, (last - first) // (n_buckets + 7) + 13, n_buckets


def test_tier_c_masks_and_aggregates_past_two_to_the_32_rows(hip, tier_c):
    streams, devs = tier_c
    cpu, gpu = _Clock(("C", "cpu")), _Clock(("C", "gpu"))
    origin, width, n_buckets = _bucket_request(streams[0])
    giant_span = sc.TIER_C["giant_points"] * sc.GIANT_DELTA
    assert width % giant_span != 0 and width > giant_span
    # the whole axis, and a range that clips a giant of either field mid-way at both ends (one end in the tail)
    tail_start = int(streams[0].batch.start_time[N_GIANTS])
    clipped = (100 * giant_span + giant_span // 3 + 5, tail_start + 40_000)
    masks = {}
    for name, (t_lo, t_hi) in (("whole", (I64_MIN, I64_MAX)), ("clipped", clipped)):
        with cpu:
            flt = mdb.value_filter(lo=0.0, t_lo=t_lo, t_hi=t_hi)
            expected = sc.streamed_filter(streams[0], flt, origin, width, n_buckets)
        n_rows = expected["n_rows"]
        # the tail's first row lies beyond 2^32, under either range
        assert int(expected["first_row"][N_GIANTS]) > (1 << 32) and (name != "whole" or n_rows % 64 != 0)
        assert 0.2 < expected["mask"].count() / n_rows < 0.8  # (PMC values and Swing spans straddle the bound)
        mask = DeviceMask(hip, n_rows)
        try:
            with gpu:
                assert hip.mask_filter_dev(devs[0], flt, mask.pointer, mask.words) == (n_rows, expected["mask"].count()), name
                mask.check(expected["mask"].bytes, ("mask", name))
                state = hip.agg_filter_dev(devs[0], flt, ALL)
                got_cells = _cells_of_one_group(hip, devs[0], flt, origin, width, n_buckets)
            sc.check_agg(state, expected["agg"], ("agg_filter", name))
            sc.check_cells(got_cells, *expected["cells"], ("buckets_filter", name))
            assert (expected["cells"][0]["count"] > 0).sum() > n_buckets // 2
            # field 1 (cut at other boundaries) under this mask
            with cpu:
                total, _ = sc.streamed_under_mask(streams[1], expected["mask"], t_lo, t_hi)
            with gpu:
                state = hip.agg_mask_dev(devs[1], t_lo, t_hi, mask.pointer, n_rows, ALL)
            sc.check_agg(state, total, ("agg_mask", name))
        finally:
            mask.free()
        if name == "whole":
            masks["a"] = expected["mask"]
    # plain per-bucket aggregates of field 1, and its own mask; then every op on the two masks
    with cpu:
        flt_b = mdb.value_filter(hi=10.0)
        every = sc.streamed_filter(streams[1], mdb.value_filter(), origin, width, n_buckets)
        expected_b = sc.streamed_filter(streams[1], flt_b)
    with gpu:
        got_cells = _cells_of_one_group(hip, devs[1], None, origin, width, n_buckets)
    sc.check_cells(got_cells, *every["cells"], "buckets")
    n_rows = every["n_rows"]
    assert every["mask"].count() == n_rows and expected_b["n_rows"] == n_rows == masks["a"].n_rows
    del every
    mask_b, out = DeviceMask(hip, n_rows), DeviceMask(hip, n_rows)
    pointer_a = hip.upload_array(masks["a"].bytes)
    try:
        with gpu:
            assert hip.mask_filter_dev(devs[1], flt_b, mask_b.pointer, mask_b.words) == (n_rows, expected_b["mask"].count())
            mask_b.check(expected_b["mask"].bytes, "mask b")
        words_a, words_b = masks["a"].words, expected_b["mask"].words
        for op, combine in WORD_OPS.items():
            with cpu:
                expected = combine(words_a, words_b)
                set_bits = sc._popcount_bytes(expected.view(np.uint8))
            with gpu:
                assert hip.mask_combine_dev(op, pointer_a, mask_b.pointer, out.pointer, n_rows) == set_bits, op
                out.check(expected.view(np.uint8), ("combine", op))
        with cpu:
            expected = ~words_a
            expected[-1] &= np.uint64((1 << (n_rows % 64)) - 1)
        with gpu:
            assert hip.mask_combine_dev(MDB_MASK_NOT, pointer_a, None, out.pointer, n_rows) == n_rows - masks["a"].count()
            out.check(expected.view(np.uint8), "not")
    finally:
        for mask in (mask_b, out):
            mask.free()
        hip.dev_free(pointer_a)


def _sparse_rows(streamed, first_row, rng):
    """A few thousand rows over the whole range: random ones, the giants' first and last rows here and there, and five
    rows of every per-point segment of the tail (MacaqueV, residual tails, irregular timestamps)."""
    n_rows = int(first_row[-1])
    rows = [rng.integers(0, n_rows, 2500), first_row[:N_GIANTS:97], first_row[1:N_GIANTS:89] - 1, [n_rows - 1, 0]]
    per_point = np.flatnonzero(sc.per_point_segments(streamed.batch))
    assert len(per_point) > 10 and per_point.min() >= N_GIANTS
    for i in per_point:
        rows.append(first_row[i] + rng.integers(0, int(streamed.lengths[i]), 5))
    return np.unique(np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]))


def test_tier_c_rows_under_sparse_and_dense_masks_and_a_filter(hip, tier_c):
    streams, devs = tier_c
    cpu, gpu = _Clock(("C", "cpu")), _Clock(("C", "gpu"))
    target, dev = streams[1], devs[1]
    rng = np.random.default_rng(12)
    with cpu:
        lengths = target.lengths
        first_row = np.concatenate([[0], np.cumsum(lengths)])
        n_rows = int(first_row[-1])
        picked = _sparse_rows(target, first_row, rng)
        sparse = sc.PackedMask(n_rows)
        for row in picked:
            sparse.set_bits(int(row), [True])
        exp_ts, exp_values, segment = sc.streamed_rows_at(target, first_row, picked)
        exp_rows = np.bincount(segment, minlength=len(target)).astype(np.uint32)
    assert int(first_row[N_GIANTS + 1]) > (1 << 32) and (picked > (1 << 32)).sum() > 100 and sparse.count() == len(picked)
    pointer = hip.upload_array(sparse.bytes)
    dense = DeviceMask(hip, n_rows)
    try:
        # a sparse mask: segment_row exceeds 2^32 in the per-point kernels
        with gpu:
            ts, values, rows, metrics = hip.grid_mask_resident(dev, I64_MIN, I64_MAX, pointer, n_rows, len(picked))
        assert np.array_equal(ts, exp_ts) and np.array_equal(values.view(np.uint32), exp_values.view(np.uint32))
        assert np.array_equal(rows, exp_rows) and metrics["rows_created"] == len(picked)
        for name, count in _rows_by_type(target.batch, exp_rows).items():
            assert metrics[f"rows_created_by_{name}"] == count, name
        # its complement: the OUTPUT exceeds 2^32 rows (values only), checked in downloaded windows
        with gpu:
            assert hip.mask_combine_dev(MDB_MASK_NOT, pointer, None, dense.pointer, n_rows) == n_rows - len(picked)
        n_out = n_rows - len(picked)
        assert n_out > (1 << 32)
        out_values, out_rows = hip.dev_alloc(4 * n_out), hip.dev_alloc(4 * len(target))
        try:
            with gpu:
                produced, metrics = hip.grid_mask_dev(dev, I64_MIN, I64_MAX, dense.pointer, n_rows, None, out_values, n_out, out_rows)
                got_rows = hip.download_array(out_rows, len(target), np.uint32)
            assert produced == n_out and metrics["rows_created"] == n_out
            assert np.array_equal(got_rows, (lengths - exp_rows).astype(np.uint32))
            out_of = lambda row: row - np.searchsorted(picked, row)  # the output position of a selected input row
            starts = [0, (1 << 31) - 2048, (1 << 32) - 2048, n_out - 4096]
            starts += [max(int(out_of(first_row[i])) - 2048, 0) for i in range(500, len(target), 500)]
            starts += [max(int(out_of(first_row[i])) - 2048, 0) for i in (N_GIANTS, N_GIANTS + 1, len(target) - 1)]
            for at in starts:
                count = min(4096, n_out - at)
                with cpu:  # the input rows behind output rows at .. at + count - 1
                    candidates = np.arange(at, at + count + len(picked), dtype=np.int64)
                    candidates = candidates[(candidates < n_rows) & ~np.isin(candidates, picked)]
                    position = out_of(candidates)
                    inputs = candidates[(position >= at) & (position < at + count)]
                    assert len(inputs) == count and position[position >= at][0] == at
                    _, expected, _ = sc.streamed_rows_at(target, first_row, inputs)
                with gpu:
                    got = hip.download_array(out_values, count, np.float32, offset_elements=at)
                assert np.array_equal(got.view(np.uint32), expected.view(np.uint32)), at
        finally:
            hip.dev_free(out_values)
            hip.dev_free(out_rows)
    finally:
        dense.free()
        hip.dev_free(pointer)
    # a filter only the tail and a few giants pass: the filtered grid writes behind 2^32 input rows
    with cpu:
        flt = mdb.value_filter(lo=90.0)
        expected = sc.streamed_filter(streams[0], flt, want_rows=True)
    passing_giants = int((expected["rows_per_segment"][:N_GIANTS] > 0).sum())
    assert 3 <= passing_giants <= 60 and (expected["rows_per_segment"][N_GIANTS:] > 0).sum() > 10
    partly = (expected["rows_per_segment"][:N_GIANTS] > 0) & (expected["rows_per_segment"][:N_GIANTS] < sc.TIER_C["giant_points"])
    assert partly.sum() >= 3  # (Swing giants whose span straddles the bound)
    with gpu:
        assert hip.grid_count_filter_dev(devs[0], flt) == len(expected["ts"])
        ts, values, rows, metrics = hip.grid_filter_resident(devs[0], flt)
    assert np.array_equal(ts, expected["ts"]) and np.array_equal(values.view(np.uint32), expected["values"].view(np.uint32))
    assert np.array_equal(rows, expected["rows_per_segment"]) and metrics["rows_created"] == len(expected["ts"])
