"""Row masks on segments (mdb_mask_filter_dev, mdb_mask_combine_dev, mdb_grid_batch_mask_dev, mdb_agg_batch_mask_dev,
mdb_agg_batch_where, mdb_grid_batch_where_owned) against the reference's plan GridExec per field -> SortedJoinExec ->
FilterExec (-> AggregateExec): the oracle's grid of every field, numpy masks with the totalOrder key on the predicate
fields' values (as tests/test_gpu_value_filter.py builds them) combined with numpy & | ^ ~, applied to the oracle's grid
of the target field. Mask bits, n_rows, n_set, padding, rows, values, rows_per_segment and the row counters bit for
bit; COUNT / MIN / MAX exact, SUM within 1e-5 of the sum of magnitudes. Expected values never come from the library
under test, except in the tests that say they are consistency checks."""

import ctypes

import numpy as np
import pytest

import cases
import datagen
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import (MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM, MDB_MASK_AND, MDB_MASK_ANDNOT,
                              MDB_MASK_NOT, MDB_MASK_OR, MDB_MASK_XOR)

pytestmark = pytest.mark.gpu

ALL = MDB_AGG_COUNT | MDB_AGG_MIN | MDB_AGG_MAX | MDB_AGG_SUM
SUM_TOLERANCE = 1e-5  # of the sum of magnitudes: the tolerance of tests/test_gpu_value_filter.py
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
F32_MAX = np.float32(np.finfo(np.float32).max)
NP_OPS = {MDB_MASK_AND: lambda a, b: a & b, MDB_MASK_OR: lambda a, b: a | b, MDB_MASK_XOR: lambda a, b: a ^ b,
          MDB_MASK_ANDNOT: lambda a, b: a & ~b}


@pytest.fixture(scope="module")
def context():
    ctx = mdb.Context(0)
    yield ctx
    for fields in _TABLES.values():  # (the resident copies _devs made on this context)
        for field in fields:
            if field.dev is not None:
                field.dev.free()
                field.dev = None
    ctx.close()


# ---- the tables: several series, every field compressed on its own under its own error bound -------------------------

class Field:
    """One field column of a table: its segments (all series, in series order) and the oracle's grid of them."""

    def __init__(self, batch, series_segments=()):
        self.batch = batch
        self.series_segments = list(series_segments)  # segments of every series, in series order
        self.ts, self.values, self.rows, _ = ora.grid_batch(batch)
        self.segment = np.repeat(np.arange(len(batch)), self.rows.astype(np.int64))
        self.dev = None

    def in_range(self, t_lo, t_hi):
        return (self.ts >= t_lo) & (self.ts <= t_hi)


def _table(series, bounds):
    """series: [(timestamps, [values of field 0, values of field 1, ...])]; bounds: one error bound per field."""
    fields = []
    for f, eb in enumerate(bounds):
        parts = [ora.try_compress_univariate_time_series(ts, values[f], eb) for ts, values in series]
        fields.append(Field(mdb.SegmentBatch.concat(parts), [len(part) for part in parts]))
    return fields


def _series(length, irregular, seeds, segment_length_range=(50, 501), t0=0):
    """One timestamp array and one value array per seed (different structures: runs of constant / linear / random)."""
    timestamps = None
    values = []
    for seed in seeds:
        ts, v = datagen.generate_univariate_time_series(length, segment_length_range, irregular, (1.0, 1.05), (100.0, 200.0),
                                                        seed)
        timestamps = ts if timestamps is None else timestamps
        values.append(v)
    return timestamps + t0, values


_TABLES = {}


def main_table():
    """Three fields (lossless, 1 % relative, absolute 5) of four series: regular and irregular timestamps, a sine with
    segments far longer than 64 rows, runs of 2..12 points with segments far shorter."""
    if "main" not in _TABLES:
        sine_ts = 5_000 + np.arange(12_000, dtype=np.int64) * 100
        sines = [datagen.sine_series(k, 12_000)[1] for k in (3, 4, 5)]
        series = [_series(6000, False, (11, 12, 13)), _series(5000, True, (21, 22, 23), t0=30_000),
                  (sine_ts, sines), _series(1500, False, (31, 32, 33), segment_length_range=(2, 12), t0=700_000)]
        bounds = cases.error_bounds()
        _TABLES["main"] = _table(series, [bounds["lossless"], bounds["rel1"], bounds["abs5"]])
    return _TABLES["main"]


def edge_table():
    """cases.edge_case_batch() (NaN, +-0, +-inf, epoch-scale Swing) and its partner: the same series under absolute 5."""
    if "edge" not in _TABLES:
        _TABLES["edge"] = [Field(cases.edge_case_batch()), Field(cases.edge_case_batch(cases.error_bounds()["abs5"]))]
    return _TABLES["edge"]


EDGE_EPOCH = 1658671178037  # the first timestamp of the edge cases' epoch-scale series


def time_ranges(fields):
    """The whole axis, a range that clips segments of every field mid-way, a range that matches nothing."""
    ts = fields[0].ts
    first, last = int(ts.min()), int(ts.max())
    if fields is _TABLES.get("edge"):  # (its series share the first second, and one reaches to 2^41)
        return [(I64_MIN, I64_MAX), (150, 950), (EDGE_EPOCH + 100_500, EDGE_EPOCH + 300_400), (last + 10, last + 1000)]
    lo, hi = first + (last - first) // 5 + 37, last - (last - first) // 3 - 11
    return [(I64_MIN, I64_MAX), (lo, hi), (last + 10, last + 1000)]


def _assert_lined_up(fields, ranges):
    """The precondition of the data: the oracle alone gives the same rows (count and timestamps) for every field."""
    for t_lo, t_hi in ranges:
        picked = [field.ts[field.in_range(t_lo, t_hi)] for field in fields]
        for other in picked[1:]:
            assert len(other) == len(picked[0]) and np.array_equal(other, picked[0])


def _devs(context, fields):
    for field in fields:
        if field.dev is None:
            field.dev = context.upload_segments(field.batch)
    return fields


def _keys(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def _key_bounds(flt):
    lo_bits, hi_bits = mdb.value_filter_bits(flt)
    lo = -(1 << 31) if flt.flags & 4 else int(_keys(np.uint32(lo_bits).view(np.float32))) + (1 if flt.flags & 1 else 0)
    hi = (1 << 31) - 1 if flt.flags & 8 else int(_keys(np.uint32(hi_bits).view(np.float32))) - (1 if flt.flags & 2 else 0)
    return lo, hi


def np_mask(field, flt, t_lo=None, t_hi=None):
    """The rows of the field's grid inside the time range (the filter's unless given): does the value pass?"""
    t_lo = flt.t_lo if t_lo is None else t_lo
    t_hi = flt.t_hi if t_hi is None else t_hi
    lo, hi = _key_bounds(flt)
    keys = _keys(field.values[field.in_range(t_lo, t_hi)])
    return (keys >= lo) & (keys <= hi)


def expected_rows(field, t_lo, t_hi, mask):
    """(timestamps, values, rows_per_segment) of the field's grid inside the range under the numpy mask."""
    inside = field.in_range(t_lo, t_hi)
    assert len(mask) == int(inside.sum())
    ts, values, segment = field.ts[inside][mask], field.values[inside][mask], field.segment[inside][mask]
    return ts, values, np.bincount(segment, minlength=len(field.batch)).astype(np.uint32)


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


class DeviceMask:
    """Device words for a mask over n_rows rows plus one guard word behind them, all pre-filled with 0xFF."""

    def __init__(self, context, n_rows):
        self.context, self.n_rows, self.words = context, n_rows, mdb.mask_words(n_rows)
        self.pointer = context.upload_array(np.full((self.words + 1) * 8, 0xFF, dtype=np.uint8))

    def check(self, expected, what):
        """The bits are `expected`, the padding bits are zero, the guard word is untouched."""
        raw = self.context.download_array(self.pointer, (self.words + 1) * 8, np.uint8)
        assert (raw[self.words * 8:] == 0xFF).all(), ("guard word", what)
        bits = mdb.unpack_mask(raw[: self.words * 8], self.words * 64)
        assert np.array_equal(bits[: self.n_rows], expected), what
        assert not bits[self.n_rows:].any(), ("padding", what)

    def free(self):
        self.context.dev_free(self.pointer)


def _filters_for(field):
    """Bounds that pass everything, nothing, about half, a sliver, and bounds on a rebuilt value (open and closed)."""
    finite = field.values[np.isfinite(field.values)]
    median = float(np.median(finite)) if len(finite) else 0.0
    picked = float(finite[len(finite) // 3]) if len(finite) else 1.0
    return [dict(), dict(lo=1e39), dict(lo=median), dict(hi=median, hi_open=True), dict(lo=picked, hi=picked),
            dict(lo=picked, lo_open=True), dict(lo=float(np.percentile(finite, 99)) if len(finite) else 0.0),
            dict(lo=median - 3.0, hi=median + 3.0)]


# ---- the data's precondition and shape ---------------------------------------------------------------------------------

def test_tables_line_up_and_cover_the_model_types():
    fields = main_table()
    _assert_lined_up(fields, time_ranges(fields))
    _assert_lined_up(edge_table(), time_ranges(edge_table()))
    # boundaries and model types differ across the fields
    assert len({len(field.batch) for field in fields}) == len(fields)
    metrics = [ora.grid_batch(field.batch)[3] for field in fields]
    assert any(all(m[f"segments_with_{name}"] > 0 for name in mdb.MODEL_TYPE_NAMES) and m["segments_with_residuals"] > 0
               for m in metrics), metrics
    rows = np.concatenate([field.rows for field in fields])
    assert rows.min() < 8 and rows.max() > 640  # far shorter and far longer than a word
    for t_lo, t_hi in time_ranges(fields)[:2]:
        assert int(fields[0].in_range(t_lo, t_hi).sum()) % 64 != 0


# ---- producing -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", ["main", "edge"])
def test_mask_bits_match_numpy(context, table):
    fields = _devs(context, main_table() if table == "main" else edge_table())
    for f, field in enumerate(fields):
        for t_lo, t_hi in time_ranges(fields):
            n_rows = int(field.in_range(t_lo, t_hi).sum())
            mask = DeviceMask(context, n_rows)
            try:
                for spec in _filters_for(field):
                    flt = mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **spec)
                    expected = np_mask(field, flt)
                    # (the buffer keeps what the previous filter left in it: the call rewrites every word it owns)
                    got_rows, got_set = context.mask_filter_dev(field.dev, flt, mask.pointer, mask.words)
                    assert (got_rows, got_set) == (n_rows, int(expected.sum())), (table, f, spec, t_lo)
                    mask.check(expected, (table, f, spec, t_lo))
                rows_only, no_set = context.mask_filter_dev(field.dev, mdb.value_filter(t_lo=t_lo, t_hi=t_hi), mask.pointer,
                                                            mask.words + 1, want_set=False)
                assert (rows_only, no_set) == (n_rows, None)
            finally:
                mask.free()


def test_edge_case_filters_nan_inf_and_zeros(context):
    fields = _devs(context, edge_table())
    nan, inf = float("nan"), float("inf")
    specs = [dict(lo=0.0), dict(hi=-0.0), dict(lo=-0.0, hi=0.0), dict(lo=inf), dict(hi=-inf), dict(lo=nan),
             dict(lo=-inf, hi=inf), dict(lo=0.0, lo_open=True, hi=inf), dict(lo=37.0, hi=73.0, hi_open=True),
             dict(lo=3.0, hi=2.0), dict(lo=5.0, t_lo=150, t_hi=950)]
    for f, field in enumerate(fields):
        for spec in specs:
            flt = mdb.value_filter(**spec)
            expected = np_mask(field, flt)
            mask = DeviceMask(context, len(expected))
            try:
                assert context.mask_filter_dev(field.dev, flt, mask.pointer, mask.words) == (len(expected), int(expected.sum()))
                mask.check(expected, (f, spec))
            finally:
                mask.free()


# ---- combining -----------------------------------------------------------------------------------------------------------

def test_combine_every_op_against_numpy(context):
    fields = main_table()
    for t_lo, t_hi in time_ranges(fields):
        a_bits = np_mask(fields[0], mdb.value_filter(lo=float(np.median(fields[0].values)), t_lo=t_lo, t_hi=t_hi))
        b_bits = np_mask(fields[1], mdb.value_filter(hi=float(np.median(fields[1].values)), t_lo=t_lo, t_hi=t_hi))
        n_rows = len(a_bits)
        for op, combine in NP_OPS.items():
            expected = combine(a_bits, b_bits)
            for alias in ("none", "a", "b"):
                a, b = context.upload_mask(a_bits), context.upload_mask(b_bits)
                out = DeviceMask(context, n_rows)
                try:
                    target = {"none": out.pointer, "a": a, "b": b}[alias]
                    assert context.mask_combine_dev(op, a, b, target, n_rows) == int(expected.sum()), (op, alias)
                    assert np.array_equal(context.download_mask(target, n_rows), expected), (op, alias)
                    assert not context.download_mask(target, n_rows, with_padding=True)[n_rows:].any(), (op, alias)
                    if alias == "none":
                        out.check(expected, (op, t_lo))
                finally:
                    out.free()
                    context.dev_free(a)
                    context.dev_free(b)
        # NOT: the tail is cleared; twice is the identity (out of place, then in place)
        a = context.upload_mask(a_bits)
        out = DeviceMask(context, n_rows)
        try:
            assert context.mask_combine_dev(MDB_MASK_NOT, a, None, out.pointer, n_rows) == int((~a_bits).sum())
            out.check(~a_bits, ("not", t_lo))
            assert context.mask_combine_dev(MDB_MASK_NOT, out.pointer, None, out.pointer, n_rows) == int(a_bits.sum())
            out.check(a_bits, ("not not", t_lo))
        finally:
            out.free()
            context.dev_free(a)


# ---- consuming: rows ---------------------------------------------------------------------------------------------------

def _check_grid_mask(context, target, t_lo, t_hi, bits, what):
    exp_ts, exp_val, exp_rows = expected_rows(target, t_lo, t_hi, bits)
    pointer = context.upload_mask(bits)
    try:
        ts, values, rows, metrics = context.grid_mask_resident(target.dev, t_lo, t_hi, pointer, len(bits), int(bits.sum()))
        cases.assert_grid_equal((ts, values), (exp_ts, exp_val))
        assert np.array_equal(rows, exp_rows), what
        assert metrics["rows_created"] == len(exp_ts), what
        for k, name in enumerate(mdb.MODEL_TYPE_NAMES):
            assert metrics[f"rows_created_by_{name}"] == int(exp_rows[target.batch.model_type_id == k].sum()), (what, name)
        no_ts, only_values, only_rows, _ = context.grid_mask_resident(target.dev, t_lo, t_hi, pointer, len(bits),
                                                                      int(bits.sum()), values_only=True)
        assert no_ts is None and np.array_equal(only_rows, exp_rows), what
        assert np.array_equal(only_values.view(np.uint32), exp_val.view(np.uint32)), what
    finally:
        context.dev_free(pointer)


def _special_masks(target, t_lo, t_hi):
    """Empty, full, alternating bits, a single bit in the middle of the longest Swing segment inside the range."""
    inside = target.in_range(t_lo, t_hi)
    n = int(inside.sum())
    out = {"empty": np.zeros(n, dtype=bool), "full": np.ones(n, dtype=bool), "alternating": np.arange(n) % 2 == 0}
    segment = target.segment[inside]
    counts = np.bincount(segment, minlength=len(target.batch))
    swing = np.where(target.batch.model_type_id == mdb.MDB_SWING_ID, counts, 0)
    if swing.max() > 0:
        rows_of = np.flatnonzero(segment == int(np.argmax(swing)))
        single = np.zeros(n, dtype=bool)
        single[rows_of[len(rows_of) // 2]] = True
        out["single"] = single
    return out


@pytest.mark.parametrize("table", ["main", "edge"])
def test_grid_mask_matches_the_oracle_under_the_numpy_mask(context, table):
    fields = _devs(context, main_table() if table == "main" else edge_table())
    for t, target in enumerate(fields):
        pred = fields[(t + 1) % len(fields)]
        for t_lo, t_hi in time_ranges(fields):
            for spec in _filters_for(pred)[:5]:
                bits = np_mask(pred, mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **spec))
                _check_grid_mask(context, target, t_lo, t_hi, bits, (table, t, spec, t_lo))
            for name, bits in _special_masks(target, t_lo, t_hi).items():
                _check_grid_mask(context, target, t_lo, t_hi, bits, (table, t, name, t_lo))


# ---- consuming: aggregates ---------------------------------------------------------------------------------------------

def _check_agg_mask(context, target, t_lo, t_hi, bits, what):
    _, exp_val, _ = expected_rows(target, t_lo, t_hi, bits)
    pointer = context.upload_mask(bits)
    try:
        state = context.agg_mask_dev(target.dev, t_lo, t_hi, pointer, len(bits), ALL)
        _check_agg(state, _expected_agg(exp_val), what)
        if not bits.any():  # no selected point: a pre-filled state stays as it is, byte for byte
            before = mdb._abi.AggStateC(1.5, 3, 2.0, 4.0)
            after = context.agg_mask_dev(target.dev, t_lo, t_hi, pointer, len(bits), ALL, mdb._abi.AggStateC(1.5, 3, 2.0, 4.0))
            assert _state_bits(after) == _state_bits(before), what
        return state
    finally:
        context.dev_free(pointer)


@pytest.mark.parametrize("table", ["main", "edge"])
def test_agg_mask_matches_the_oracle_under_the_numpy_mask(context, table):
    fields = _devs(context, main_table() if table == "main" else edge_table())
    singles = 0
    for t, target in enumerate(fields):
        pred = fields[(t + 1) % len(fields)]
        for t_lo, t_hi in time_ranges(fields):
            for spec in _filters_for(pred):
                bits = np_mask(pred, mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **spec))
                _check_agg_mask(context, target, t_lo, t_hi, bits, (table, t, spec, t_lo))
            specials = _special_masks(target, t_lo, t_hi)
            singles += "single" in specials
            for name, bits in specials.items():
                _check_agg_mask(context, target, t_lo, t_hi, bits, (table, t, name, t_lo))
    assert singles > 0
    if table == "main":  # the single bit sat in a long Swing segment
        target = fields[1]
        inside = target.in_range(I64_MIN, I64_MAX)
        counts = np.bincount(target.segment[inside], minlength=len(target.batch))
        assert np.where(target.batch.model_type_id == mdb.MDB_SWING_ID, counts, 0).max() > 200


# ---- the host forms ----------------------------------------------------------------------------------------------------

def _where_expected(target, preds, filters):
    """The intersection of the filters' time ranges, the ANDed numpy masks over it, and the target's rows under them."""
    t_lo = max([flt.t_lo for flt in filters], default=I64_MIN)
    t_hi = min([flt.t_hi for flt in filters], default=I64_MAX)
    bits = np.ones(int(target.in_range(t_lo, t_hi).sum()), dtype=bool)
    for field, flt in zip(preds, filters):
        bits &= np_mask(field, flt, t_lo, t_hi)
    return t_lo, t_hi, bits, expected_rows(target, t_lo, t_hi, bits)


def _check_where(context, target, preds, filters, what):
    t_lo, t_hi, bits, (exp_ts, exp_val, exp_rows) = _where_expected(target, preds, filters)
    batches = [field.batch for field in preds]
    state = context.agg_where(batches, filters, target.batch, ALL)
    _check_agg(state, _expected_agg(exp_val), what)
    ts, values, rows, metrics = context.grid_where(batches, filters, target.batch)
    cases.assert_grid_equal((ts, values), (exp_ts, exp_val))
    assert np.array_equal(rows, exp_rows) and metrics["rows_created"] == len(exp_ts), what
    no_ts, only_values, only_rows, _ = context.grid_where(batches, filters, target.batch, values_only=True, reserve_front=5)
    assert no_ts is None and np.array_equal(only_rows, exp_rows), what
    assert np.array_equal(only_values.view(np.uint32), exp_val.view(np.uint32)), what
    return t_lo, t_hi, bits, state, (ts, values, rows, metrics)


def test_where_two_and_three_predicates_with_differing_time_ranges(context):
    fields = main_table()
    (_, _), (lo, hi), _ = time_ranges(fields)
    span = hi - lo
    m = [float(np.median(field.values)) for field in fields]
    cases_ = [
        (fields[2], [fields[0], fields[1]],
         [mdb.value_filter(lo=m[0], t_lo=lo, t_hi=hi), mdb.value_filter(hi=m[1] + 4.0, t_lo=lo + span // 7, t_hi=I64_MAX)]),
        (fields[0], [fields[0], fields[1], fields[2]],  # the target is a predicate field
         [mdb.value_filter(lo=m[0] - 2.0), mdb.value_filter(lo=m[1] - 6.0, t_hi=hi - span // 9),
          mdb.value_filter(hi=m[2] + 6.0, hi_open=True, t_lo=lo + 13)]),
        (fields[1], [fields[1]], [mdb.value_filter(lo=m[1], lo_open=True)]),
        (fields[1], [fields[2], fields[2]],  # the same field twice: a BETWEEN written as two predicates
         [mdb.value_filter(lo=m[2] - 1.0), mdb.value_filter(hi=m[2] + 1.0, t_lo=lo)]),
        (fields[2], [fields[0], fields[1]],  # an empty intersection selects nothing
         [mdb.value_filter(t_lo=lo, t_hi=lo + 100), mdb.value_filter(t_lo=lo + 200, t_hi=hi)]),
        (fields[2], [fields[0]], [mdb.value_filter(t_lo=hi + 10**9, t_hi=hi + 2 * 10**9)]),  # a range matching nothing
        (fields[0], [], []),  # no predicate: every row of the whole time axis
    ]
    for k, (target, preds, filters) in enumerate(cases_):
        _check_where(context, target, preds, filters, k)
    edge = edge_table()
    for target, pred in ((edge[0], edge[1]), (edge[1], edge[0])):
        for spec in (dict(lo=0.0), dict(lo=float("nan")), dict(hi=37.0, t_lo=150, t_hi=950), dict(lo=-0.0, hi=0.0)):
            _check_where(context, target, [pred], [mdb.value_filter(**spec)], spec)


# ---- consistency between the routes (these compare entry points of the library with each other, on purpose) ---------

def test_consistency_with_the_filtered_calls_and_between_routes(context):
    """Consistency check: a mask made from the target field's own filter gives grid_mask == grid_filter_resident bit
    for bit and agg_mask COUNT / MIN / MAX == agg_filter_dev; the dev route equals the *_where host route bit for bit;
    two runs agree bit for bit."""
    for fields in (main_table(), edge_table()):
        _devs(context, fields)
        for target in fields:
            for t_lo, t_hi in time_ranges(fields)[:2]:
                flt = mdb.value_filter(lo=float(np.median(target.values[np.isfinite(target.values)])), t_lo=t_lo, t_hi=t_hi)
                n_rows = int(target.in_range(t_lo, t_hi).sum())
                mask = DeviceMask(context, n_rows)
                try:
                    _, n_set = context.mask_filter_dev(target.dev, flt, mask.pointer, mask.words)
                    masked = context.grid_mask_resident(target.dev, t_lo, t_hi, mask.pointer, n_rows, n_set)
                    filtered = context.grid_filter_resident(target.dev, flt)
                    cases.assert_grid_equal(masked, filtered)
                    assert np.array_equal(masked[2], filtered[2]) and masked[3] == filtered[3]
                    state = context.agg_mask_dev(target.dev, t_lo, t_hi, mask.pointer, n_rows, ALL)
                    reference = context.agg_filter_dev(target.dev, flt, ALL)
                    assert state.count == reference.count and _same_float(state.min, reference.min)
                    assert _same_float(state.max, reference.max)
                    again = context.agg_mask_dev(target.dev, t_lo, t_hi, mask.pointer, n_rows, ALL)
                    host = context.agg_where([target.batch], [flt], target.batch, ALL)
                    assert _state_bits(state) == _state_bits(again) == _state_bits(host)
                    rows_host = context.grid_where([target.batch], [flt], target.batch)
                    cases.assert_grid_equal(rows_host, masked)
                    assert np.array_equal(rows_host[2], masked[2]) and rows_host[3] == masked[3]
                finally:
                    mask.free()
    # two predicates over two fields: masks made and ANDed by hand on the device against the host form
    fields = main_table()
    (_, _), (t_lo, t_hi), _ = time_ranges(fields)
    filters = [mdb.value_filter(lo=float(np.median(fields[0].values)), t_lo=t_lo, t_hi=t_hi),
               mdb.value_filter(hi=float(np.median(fields[1].values)), t_lo=t_lo, t_hi=t_hi)]
    n_rows = int(fields[2].in_range(t_lo, t_hi).sum())
    a, b = DeviceMask(context, n_rows), DeviceMask(context, n_rows)
    try:
        context.mask_filter_dev(fields[0].dev, filters[0], a.pointer, a.words)
        context.mask_filter_dev(fields[1].dev, filters[1], b.pointer, b.words)
        n_set = context.mask_combine_dev(MDB_MASK_AND, a.pointer, b.pointer, a.pointer, n_rows)
        dev_state = context.agg_mask_dev(fields[2].dev, t_lo, t_hi, a.pointer, n_rows, ALL)
        host_state = context.agg_where([fields[0].batch, fields[1].batch], filters, fields[2].batch, ALL)
        assert _state_bits(dev_state) == _state_bits(host_state)
        dev_rows = context.grid_mask_resident(fields[2].dev, t_lo, t_hi, a.pointer, n_rows, n_set)
        host_rows = context.grid_where([fields[0].batch, fields[1].batch], filters, fields[2].batch)
        cases.assert_grid_equal(dev_rows, host_rows)
        assert np.array_equal(dev_rows[2], host_rows[2]) and dev_rows[3] == host_rows[3]
    finally:
        a.free()
        b.free()


def test_several_slices_under_a_scratch_limit(context):
    """The per-point segments rebuilt in several slices (producer and consumer) give the same bits and rows."""
    fields = main_table()
    t_lo, t_hi = time_ranges(fields)[1]
    ctx = mdb.Context(0)
    devs = []
    try:
        ctx.set_scratch_limit(1 << 16)  # slices of 1365 points
        devs = [ctx.upload_segments(field.batch) for field in fields]
        flt = mdb.value_filter(lo=float(np.median(fields[0].values)), t_lo=t_lo, t_hi=t_hi)
        expected = np_mask(fields[0], flt)
        mask = DeviceMask(ctx, len(expected))
        try:
            assert ctx.mask_filter_dev(devs[0], flt, mask.pointer, mask.words) == (len(expected), int(expected.sum()))
            mask.check(expected, "slices")
            for target, dev in zip(fields, devs):
                exp_ts, exp_val, exp_rows = expected_rows(target, t_lo, t_hi, expected)
                got = ctx.grid_mask_resident(dev, t_lo, t_hi, mask.pointer, len(expected), int(expected.sum()))
                cases.assert_grid_equal(got, (exp_ts, exp_val))
                assert np.array_equal(got[2], exp_rows)
                _check_agg(ctx.agg_mask_dev(dev, t_lo, t_hi, mask.pointer, len(expected), ALL), _expected_agg(exp_val), "slices")
        finally:
            mask.free()
    finally:
        for dev in devs:
            dev.free()
        ctx.close()


# ---- errors --------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched(context):
    fields = _devs(context, main_table())
    target, pred = fields[1], fields[0]
    t_lo, t_hi = time_ranges(fields)[1]
    flt = mdb.value_filter(lo=float(np.median(pred.values)), t_lo=t_lo, t_hi=t_hi)
    bits = np_mask(pred, flt)
    n_rows, n_set = len(bits), int(bits.sum())
    assert n_set > 1
    bad_flags = mdb.value_filter(lo=1.0)
    bad_flags.flags |= 16
    bad_reserved = mdb.value_filter(lo=1.0)
    bad_reserved.reserved = 1
    lib, handle, vp = context.lib, context.handle, ctypes.c_void_p
    # mask_filter: cap_words too small, bad flags, NULL arguments - the buffer and the counters stay as they were
    mask = DeviceMask(context, n_rows)
    try:
        for filter_, cap in ((flt, mask.words - 1), (bad_flags, mask.words), (bad_reserved, mask.words)):
            rows_out, set_out = ctypes.c_uint64(12345), ctypes.c_uint64(678)
            code = lib.mdb_mask_filter_dev(handle, ctypes.byref(pred.dev.seg), ctypes.byref(filter_), vp(mask.pointer), cap,
                                           ctypes.byref(rows_out), ctypes.byref(set_out))
            assert code != 0 and (rows_out.value, set_out.value) == (12345, 678)
            assert context.download_mask(mask.pointer, mask.words * 64).all()
        rows_out = ctypes.c_uint64(12345)
        assert lib.mdb_mask_filter_dev(handle, None, ctypes.byref(flt), vp(mask.pointer), mask.words, ctypes.byref(rows_out), None) != 0
        assert lib.mdb_mask_filter_dev(handle, ctypes.byref(pred.dev.seg), None, vp(mask.pointer), mask.words, ctypes.byref(rows_out), None) != 0
        assert lib.mdb_mask_filter_dev(handle, ctypes.byref(pred.dev.seg), ctypes.byref(flt), vp(mask.pointer), mask.words, None, None) != 0
        assert lib.mdb_mask_filter_dev(None, ctypes.byref(pred.dev.seg), ctypes.byref(flt), vp(mask.pointer), mask.words, ctypes.byref(rows_out), None) != 0
        assert rows_out.value == 12345 and context.download_mask(mask.pointer, mask.words * 64).all()
        # combine: an unknown op, b with NOT, NULL masks
        a = context.upload_mask(bits)
        try:
            for op, b in ((5, a), (77, a), (MDB_MASK_NOT, a), (MDB_MASK_AND, None)):
                set_out = ctypes.c_uint64(678)
                code = lib.mdb_mask_combine_dev(handle, op, vp(a), vp(b), vp(mask.pointer), n_rows, ctypes.byref(set_out))
                assert code != 0 and set_out.value == 678, op
            assert lib.mdb_mask_combine_dev(handle, MDB_MASK_AND, None, vp(a), vp(mask.pointer), n_rows, None) != 0
            assert lib.mdb_mask_combine_dev(handle, MDB_MASK_AND, vp(a), vp(a), None, n_rows, None) != 0
            assert lib.mdb_mask_combine_dev(None, MDB_MASK_AND, vp(a), vp(a), vp(mask.pointer), n_rows, None) != 0
            assert context.download_mask(mask.pointer, mask.words * 64).all()
            assert np.array_equal(context.download_mask(a, n_rows), bits)
        finally:
            context.dev_free(a)
    finally:
        mask.free()
    # the consumers: a row-count mismatch (the target with one series fewer; a mask of one row more), cap too small
    pointer = context.upload_mask(bits)
    sentinel_ts = np.full(n_set, -7, dtype=np.int64)
    sentinel_val = np.full(n_set, 0x5A5A5A5A, dtype=np.uint32).view(np.float32)
    sentinel_rows = np.full(len(target.batch), 0xABCD, dtype=np.uint32)
    out_ts, out_val, out_rows = (context.upload_array(x) for x in (sentinel_ts, sentinel_val, sentinel_rows))
    fewer_batch = target.batch.take(np.arange(len(target.batch) - target.series_segments[-1]))  # without the last series
    assert len(fewer_batch) < len(target.batch) and t_lo < 700_000 < t_hi  # (which reaches into the time range)
    fewer = context.upload_segments(fewer_batch)
    try:
        for dev, rows, cap in ((fewer, n_rows, n_set), (target.dev, n_rows + 1, n_set), (target.dev, n_rows, n_set - 1)):
            n_out = ctypes.c_uint64(12345)
            metrics = mdb._abi.GridMetricsC()
            code = lib.mdb_grid_batch_mask_dev(handle, ctypes.byref(dev.seg), t_lo, t_hi, vp(pointer), rows, vp(out_ts),
                                               vp(out_val), vp(out_rows), cap, ctypes.byref(n_out), ctypes.byref(metrics))
            assert code != 0 and n_out.value == 12345 and metrics.rows_created == 0
            assert np.array_equal(context.download_array(out_ts, n_set, np.int64), sentinel_ts)
            assert np.array_equal(context.download_array(out_val, n_set, np.float32).view(np.uint32), sentinel_val.view(np.uint32))
            assert np.array_equal(context.download_array(out_rows, len(target.batch), np.uint32), sentinel_rows)
        with pytest.raises(mdb.HipError, match=r"\d+ rows.*\d+ rows"):
            context.grid_mask_dev(fewer, t_lo, t_hi, pointer, n_rows, out_ts, out_val, n_set)
        before = _state_bits(mdb._abi.AggStateC(1.5, 3, 2.0, 4.0))
        for dev, rows in ((fewer, n_rows), (target.dev, n_rows + 1)):
            state = mdb._abi.AggStateC(1.5, 3, 2.0, 4.0)
            with pytest.raises(mdb.HipError, match=r"\d+ rows.*\d+ rows"):
                context.agg_mask_dev(dev, t_lo, t_hi, pointer, rows, ALL, state)
            assert _state_bits(state) == before
        state = mdb._abi.AggStateC(1.5, 3, 2.0, 4.0)
        assert lib.mdb_agg_batch_mask_dev(handle, None, t_lo, t_hi, vp(pointer), n_rows, ALL, ctypes.byref(state)) != 0
        assert lib.mdb_agg_batch_mask_dev(handle, ctypes.byref(target.dev.seg), t_lo, t_hi, None, n_rows, ALL, ctypes.byref(state)) != 0
        assert lib.mdb_agg_batch_mask_dev(handle, ctypes.byref(target.dev.seg), t_lo, t_hi, vp(pointer), n_rows, ALL, None) != 0
        assert lib.mdb_grid_batch_mask_dev(handle, None, t_lo, t_hi, vp(pointer), n_rows, vp(out_ts), vp(out_val), None, n_set, None, None) != 0
        assert lib.mdb_grid_batch_mask_dev(handle, ctypes.byref(target.dev.seg), t_lo, t_hi, None, n_rows, vp(out_ts), vp(out_val), None, n_set, None, None) != 0
        assert lib.mdb_grid_batch_mask_dev(handle, ctypes.byref(target.dev.seg), t_lo, t_hi, vp(pointer), n_rows, vp(out_ts), None, None, n_set, None, None) != 0
        assert _state_bits(state) == before
        assert np.array_equal(context.download_array(out_ts, n_set, np.int64), sentinel_ts)
        # the host forms: fields that do not line up, bad filter flags, bad flags of the owned form, NULL arguments
        for bad_target, preds, filters in ((fewer_batch, [pred.batch], [flt]), (target.batch, [fewer_batch], [flt]),
                                           (target.batch, [pred.batch], [bad_flags]), (target.batch, [pred.batch, pred.batch], [flt, bad_reserved])):
            state = mdb._abi.AggStateC(1.5, 3, 2.0, 4.0)
            with pytest.raises(mdb.HipError):
                context.agg_where(preds, filters, bad_target, ALL, state)
            assert _state_bits(state) == before
            with pytest.raises(mdb.HipError):
                context.grid_where(preds, filters, bad_target)
        for flags in (1, 3, 4, 1 << 31):
            with pytest.raises(mdb.HipError):
                context.grid_where([pred.batch], [flt], target.batch, flags=flags)
        seg = target.batch.as_c()
        pointers = (ctypes.POINTER(mdb._abi.SegmentsC) * 1)(ctypes.pointer(seg))
        out = ctypes.POINTER(mdb._abi.GridResultC)()
        state = mdb._abi.AggStateC(1.5, 3, 2.0, 4.0)
        assert lib.mdb_agg_batch_where(handle, None, ctypes.byref(flt), 1, ctypes.byref(seg), ALL, ctypes.byref(state)) != 0
        assert lib.mdb_agg_batch_where(handle, pointers, None, 1, ctypes.byref(seg), ALL, ctypes.byref(state)) != 0
        assert lib.mdb_agg_batch_where(handle, pointers, ctypes.byref(flt), 1, None, ALL, ctypes.byref(state)) != 0
        assert lib.mdb_agg_batch_where(handle, pointers, ctypes.byref(flt), 1, ctypes.byref(seg), ALL, None) != 0
        assert lib.mdb_grid_batch_where_owned(handle, pointers, ctypes.byref(flt), 1, None, 0, 0, ctypes.byref(out)) != 0
        assert lib.mdb_grid_batch_where_owned(handle, pointers, ctypes.byref(flt), 1, ctypes.byref(seg), 0, 0, None) != 0
        assert _state_bits(state) == before and not out
    finally:
        fewer.free()
        for p in (pointer, out_ts, out_val, out_rows):
            context.dev_free(p)


# ---- a seeded fuzz -------------------------------------------------------------------------------------------------------

FUZZ_TRIALS = 240


def test_seeded_fuzz(context):
    """Small tables of two fields (fixed seeds): random bounds, time ranges and ops; masks, rows and aggregates."""
    rng = np.random.default_rng(20261016)
    bounds = list(cases.error_bounds().values())
    ops = list(NP_OPS) + [MDB_MASK_NOT]
    for trial in range(FUZZ_TRIALS):
        length = int(rng.integers(40, 700))
        segment_range = (int(rng.integers(2, 40)), int(rng.integers(41, 300)))
        ts, values = _series(length, bool(rng.integers(2)), (int(rng.integers(1 << 30)), int(rng.integers(1 << 30))),
                             segment_length_range=segment_range, t0=int(rng.integers(0, 10**6)))
        fields = _table([(ts, values)], [bounds[int(rng.integers(len(bounds)))], bounds[int(rng.integers(len(bounds)))]])
        if rng.integers(2):
            t_lo, t_hi = sorted(rng.integers(int(ts[0]) - 10, int(ts[-1]) + 10, 2).tolist())
        else:
            t_lo, t_hi = I64_MIN, I64_MAX
        _assert_lined_up(fields, [(t_lo, t_hi)])
        filters = []
        for field in fields:
            pick = lambda: float(field.values[int(rng.integers(len(field.values)))])
            lo, hi = sorted([pick(), pick()])
            filters.append(mdb.value_filter(lo=lo if rng.integers(3) else None, hi=hi if rng.integers(3) else None,
                                            lo_open=bool(rng.integers(2)), hi_open=bool(rng.integers(2)), t_lo=t_lo, t_hi=t_hi))
        op = ops[int(rng.integers(len(ops)))]
        target = fields[int(rng.integers(2))]
        np_masks = [np_mask(field, flt) for field, flt in zip(fields, filters)]
        expected = ~np_masks[0] if op == MDB_MASK_NOT else NP_OPS[op](np_masks[0], np_masks[1])
        n_rows = len(expected)
        devs = [context.upload_segments(field.batch) for field in fields]
        masks = [DeviceMask(context, n_rows) for _ in fields]
        try:
            for field, dev, flt, mask, bits in zip(fields, devs, filters, masks, np_masks):
                assert context.mask_filter_dev(dev, flt, mask.pointer, mask.words) == (n_rows, int(bits.sum())), trial
                mask.check(bits, trial)
            n_set = context.mask_combine_dev(op, masks[0].pointer, None if op == MDB_MASK_NOT else masks[1].pointer,
                                             masks[0].pointer, n_rows)
            assert n_set == int(expected.sum()), trial
            masks[0].check(expected, (trial, op))
            exp_ts, exp_val, exp_rows = expected_rows(target, t_lo, t_hi, expected)
            dev = devs[fields.index(target)]
            got = context.grid_mask_resident(dev, t_lo, t_hi, masks[0].pointer, n_rows, n_set)
            cases.assert_grid_equal(got, (exp_ts, exp_val))
            assert np.array_equal(got[2], exp_rows), trial
            _check_agg(context.agg_mask_dev(dev, t_lo, t_hi, masks[0].pointer, n_rows, ALL), _expected_agg(exp_val), trial)
            if op == MDB_MASK_AND:
                _check_where(context, target, fields, filters, trial)
        finally:
            for mask in masks:
                mask.free()
            for dev in devs:
                dev.free()
