"""Derived fields of two fields on the GPU (mdb_derived_values*, mdb_derived_buckets*) through the C ABI against the
reference of tests/derived_cases.py: z by numpy float32 in the written order on the oracle's grids, per cell count, min
and max exactly (min and max with ==: the sign of a zero extreme follows the order of merges, mdb.h) and mean / m2 in
exact arithmetic around the first value.

Tolerances (the project's for this arithmetic, mdb.h and tests/test_comoments_cpu.py): the z column bit for bit; count,
min, max exact; mean within 2^-44 of the cell's largest |z|; m2 within 1e-5 of its reference. Expected values never come
from the library under test, except in the tests that say they are consistency checks."""

import ctypes

import numpy as np
import pytest

import cases
import comoments_cases as cc
import derived_cases as dc
import layouts
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

INTERVAL = dc.INTERVAL
I64_MIN, I64_MAX = dc.I64_MIN, dc.I64_MAX
CELL = mdb.DERIVED_CELL_DTYPE
SHORT, CHUNK = dc.SHORT, dc.CHUNK
_TABLES = {}


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()
    for fields in _TABLES.values():
        for field in fields:
            field.free()


def _same_bits(got, expected):
    return got.shape == expected.shape and bool(((got.view(np.uint32) == expected.view(np.uint32)) | (np.isnan(got) & np.isnan(expected))).all())


def _span(fields):
    return int(fields[0].ts.min()), int(fields[0].ts.max())


def _noise_table():
    """One series of 4 * CHUNK + 300 rows per level (0, 1e6, 1e7; sigma 0.5), lossless, x cut into 3 chunks and y into
    5: long MacaqueV streams, so the (segment, bucket) intervals are as long as the buckets make them."""
    if "noise" not in _TABLES:
        n = 4 * CHUNK + 300
        rng = np.random.default_rng(2070)
        timestamps = 1_000 + np.arange(n, dtype=np.int64) * INTERVAL
        tables = []
        for name, (xv, yv) in dc.data_sets(rng, n).items():
            x = cc.Field([ora.compress_chunks(timestamps, xv, np.array([0, 2 * CHUNK + 70, 2 * CHUNK + 71, n], dtype=np.uint64), cases.LOSSLESS)])
            y = cc.Field([ora.compress_chunks(timestamps, yv, np.array([0, 5, 900, 901, 3 * CHUNK, n], dtype=np.uint64), cases.LOSSLESS)])
            tables += [x, y]
        _TABLES["noise"] = tables
        for field in tables:
            assert len(field.ts) == n
    return [(_TABLES["noise"][k], _TABLES["noise"][k + 1]) for k in (0, 2, 4)]


def _values_dev(hip, x, y, expr, t_lo, t_hi, offset=0, timestamps=True):
    """mdb_derived_values_dev into device arrays, the values pointer `offset` floats behind a 16-byte aligned address.
    Returns (timestamps or None, z, the guard floats in front of and behind z)."""
    n = int(x.in_range(t_lo, t_hi).sum())
    dev_ts = hip.dev_alloc(8 * max(n, 1)) if timestamps else None
    guard = np.full(n + 8, -77.0, dtype=np.float32)
    dev_values = hip.upload_array(guard)
    try:
        rows = hip.derived_values_dev(x.resident(hip), y.resident(hip), dc.expression(expr), t_lo, t_hi, dev_ts,
                                      dev_values + 4 * offset, n)
        assert rows == n
        everything = hip.download_array(dev_values, n + 8, np.float32)
        ts = hip.download_array(dev_ts, n, np.int64) if timestamps and n else None
    finally:
        hip.dev_free(dev_values)
        if dev_ts is not None:
            hip.dev_free(dev_ts)
    return ts, everything[offset:offset + n], np.concatenate([everything[:offset], everything[offset + n:]])


# ---- the column ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(dc.EXPRESSIONS))
def test_the_column_is_numpys_bit_for_bit(hip, name):
    """PMC-Mean, Swing and MacaqueV, residual tails, irregular timestamps, fields cut differently; the whole range and
    one that clips the first and the last segment of a series mid-way; host form and device form."""
    fields = cc.main_table()
    first, last = _span(fields)
    for x, y in ((fields[0], fields[2]), (fields[1], fields[0])):
        for t_lo, t_hi in ((I64_MIN, I64_MAX), (first + 7_777, last - 12_321)):
            ts, z = dc.column(x, y, name, t_lo, t_hi)
            got_ts, got = hip.derived_values(x.batch, y.batch, dc.expression(name), t_lo, t_hi)
            assert np.array_equal(got_ts, ts) and _same_bits(got, z), (name, t_lo)
            dev_ts, dev, guard = _values_dev(hip, x, y, name, t_lo, t_hi)
            assert np.array_equal(dev_ts, ts) and _same_bits(dev, z) and (guard == -77.0).all(), (name, t_lo)


def test_the_column_on_special_values(hip):
    """NaN, +-0, +-inf, one- and two-point segments, epoch-scale Swing (cases.edge_case_series)."""
    x, y = cc.edge_table()
    for name in dc.EXPRESSIONS:
        for a, b in ((x, y), (y, x), (x, x)):
            ts, z = dc.column(a, b, name)
            got_ts, got = hip.derived_values(a.batch, b.batch, dc.expression(name))
            assert np.array_equal(got_ts, ts) and _same_bits(got, z), name
    assert np.isnan(x.values).any() and np.isinf(x.values).any()


@pytest.mark.parametrize("rows", [0, 1, 3, 4, 5, 255, 256, 257, 4 * CHUNK - 1, 4 * CHUNK + 2])
def test_row_counts_alignment_and_timestamps(hip, rows):
    """Row counts around the 16-byte groups and the kernel's blocks, the output pointer on and one float off a 16-byte
    boundary, with and without timestamps; x in 3 segments (or more) against y in 5."""
    x, y = _noise_table()[1]
    assert len(x.batch) != len(y.batch) and len(x.batch) >= 3 and len(y.batch) >= 5
    start = int(x.ts[7])
    t_lo, t_hi = (start, start + (rows - 1) * INTERVAL) if rows else (start + 1, start + INTERVAL - 1)
    ts, z = dc.column(x, y, "scaled_ratio", t_lo, t_hi)
    assert len(z) == rows
    for offset in (0, 1):
        for timestamps in (True, False):
            got_ts, got, guard = _values_dev(hip, x, y, "scaled_ratio", t_lo, t_hi, offset, timestamps)
            assert _same_bits(got, z) and (guard == -77.0).all(), (rows, offset, timestamps)
            assert got_ts is None or np.array_equal(got_ts, ts)


def test_macaque_v_streams_of_awkward_lengths(hip):
    timestamps = np.arange(63 + 64 + 65 + 129, dtype=np.int64) * INTERVAL
    rng = np.random.default_rng(2071)
    offsets = np.cumsum([0, 63, 64, 65, 129]).astype(np.uint64)
    x = cc.Field([ora.compress_chunks(timestamps, rng.normal(5.0, 1.0, len(timestamps)).astype(np.float32), offsets, cases.LOSSLESS)])
    y = cc.Field([ora.compress_chunks(timestamps, rng.normal(5.0, 1.0, len(timestamps)).astype(np.float32), offsets[::-1].max() - offsets[::-1], cases.LOSSLESS)])
    try:
        assert (x.batch.model_type_id == mdb.MDB_MACAQUE_V_ID).all() and sorted(x.rows.tolist()) == [63, 64, 65, 129]
        for name in ("product", "ratio"):
            _, z = dc.column(x, y, name)
            assert _same_bits(hip.derived_values(x.batch, y.batch, dc.expression(name))[1], z)
            assert _same_bits(_values_dev(hip, x, y, name, I64_MIN, I64_MAX, 1, False)[1], z)
            cells = hip.derived_buckets(x.batch, y.batch, dc.expression(name), 0, 50 * INTERVAL, 7)
            dc.assert_cells(cells, dc.oracle(x, y, name, None, 1, 0, 50 * INTERVAL, 7), name)
    finally:
        x.free()
        y.free()


# ---- the buckets --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["absolute_difference", "weighted_sum", "product", "scaled_ratio", "x_alone"])
def test_parity_with_the_points_in_exact_arithmetic(hip, name):
    """The requests of the moments tests over the main table: buckets of 1 row, buckets a segment's span reaches but no
    point lies in (irregular series), rows outside every bucket, a range that cuts buckets, four groups and one."""
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    for request, origin, width, n_buckets, t_lo, t_hi in cc.bucket_sets(*_span(fields)):
        for groups, n_groups in ((x.groups, 4), (None, 1)):
            got = hip.derived_buckets(x.batch, y.batch, dc.expression(name), origin, width, n_buckets, groups=groups,
                                      t_lo=t_lo, t_hi=t_hi, n_groups=n_groups)
            dc.assert_cells(got, dc.oracle(x, y, name, groups, n_groups, origin, width, n_buckets, t_lo, t_hi),
                            f"{name} {request} {n_groups} group(s)")
            counts = hip.agg_buckets(x.batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=n_groups)
            np.testing.assert_array_equal(got["count"], counts["count"])


def _interval_lengths(x, origin, width, n_buckets):
    buckets = (x.ts - origin) // width
    keep = (buckets >= 0) & (buckets < n_buckets)
    pairs, first, counts = np.unique(x.segment[keep] * n_buckets + buckets[keep], return_index=True, return_counts=True)
    return counts, np.flatnonzero(keep)[first]


@pytest.mark.parametrize("length", [SHORT - 1, SHORT, SHORT + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_interval_lengths_around_both_constants(hip, length, monkeypatch):
    """Buckets of `length` rows over long segments, shifted so that intervals begin at rows that are no multiple of 4:
    the levels 0, 1e6 and 1e7 with sigma 0.5, under slices of 1 and 7 entries and the default."""
    for level, (x, y) in enumerate(_noise_table()):
        first = int(x.ts[0])
        for shift in (3, 1):
            origin, width = first + shift * INTERVAL, length * INTERVAL
            n_buckets = (int(x.ts[-1]) - origin) // width + 1
            counts, starts = _interval_lengths(x, origin, width, n_buckets)
            # (at 1e7 an f32 holds whole numbers only: the values repeat, the segments are short PMC-Mean and Swing runs
            # and so are the intervals - that level checks the arithmetic, the other two the lengths)
            assert level == 2 or ((counts == length).any() and (starts[counts == length] % 4 != 0).any())
            for name in ("difference", "product") if level else ("product", "scaled_ratio"):
                expected = dc.oracle(x, y, name, None, 1, origin, width, n_buckets)
                got = hip.derived_buckets(x.batch, y.batch, dc.expression(name), origin, width, n_buckets)
                dc.assert_cells(got, expected, f"level {level} length {length} shift {shift} {name}")
                if shift == 3 and name == "product":
                    for slice_pairs in ("1", "7"):
                        monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", slice_pairs)
                        sliced = hip.derived_buckets(x.batch, y.batch, dc.expression(name), origin, width, n_buckets)
                        monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
                        dc.assert_cells(sliced, expected, f"slices of {slice_pairs}")
                        for member in ("count", "min", "max"):
                            assert sliced[member].tobytes() == got[member].tobytes()


def test_one_bucket_takes_every_chunk_of_a_long_segment(hip):
    """(also a check of the wave path itself) one bucket over everything: whole chunks and the two partial ones."""
    for x, y in _noise_table():
        first, last = _span([x])
        hip.profile_enable(True)
        hip.profile_reset()
        got = hip.derived_buckets(x.batch, y.batch, dc.expression("product"), first, last - first + 1, 1)
        kernels = hip.profile()
        hip.profile_enable(False)
        assert "k_derived_waves" in kernels and "k_derived_lanes" in kernels and "k_derived_intervals" in kernels, sorted(kernels)
        dc.assert_cells(got, dc.oracle(x, y, "product", None, 1, first, last - first + 1, 1), "one bucket")


def test_unsorted_irregular_streams_go_through_the_fallback(hip):
    """(a consistency check) Segments whose irregular timestamps are not sorted (a malformed stream that still decodes:
    the batches of tests/test_gpu_hist_buckets.py), the field paired with itself: count is mdb_agg_buckets' COUNT, x - x
    is zero everywhere, and z = x has the extremes of mdb_agg_buckets and the moments of mdb_moments_buckets."""
    from test_gpu_hist_buckets import _unsorted
    for eb_name in ("lossless", "abs5"):
        _, _, sorted_batch = cases.mixed_batch(cases.error_bounds()[eb_name], True, seed=1700 + len(eb_name), length=3_000)
        batch, changed, _ = _unsorted(sorted_batch, np.random.default_rng(17))
        assert len(changed) >= 5
        first, last = int(batch.start_time.min()), int(batch.end_time.max())
        groups = np.arange(len(batch), dtype=np.uint32) % 3
        for origin, width in ((first, (last - first) // 64 | 1), (first - 77, (last - first) // 23)):
            args = (origin, width, (last - origin) // width + 1)
            states = hip.agg_buckets(batch, *args, groups=groups, n_groups=3)
            moments = hip.moments_buckets(batch, *args, groups=groups, n_groups=3)
            zero = hip.derived_buckets(batch, batch, dc.expression("difference"), *args, groups=groups, n_groups=3)
            same = hip.derived_buckets(batch, batch, dc.expression("x_alone"), *args, groups=groups, n_groups=3)
            hit = states["count"] > 0
            assert int(states["count"].sum()) > 2_000
            for cells in (zero, same):
                np.testing.assert_array_equal(cells["count"], states["count"])
            for member in ("mean", "m2", "min", "max"):
                assert (zero[member][hit] == 0.0).all(), member
            np.testing.assert_array_equal(same["min"][hit], states["min"][hit])
            np.testing.assert_array_equal(same["max"][hit], states["max"][hit])
            largest = np.maximum(np.abs(states["min"][hit]), np.abs(states["max"][hit])).astype(np.float64)
            assert (np.abs(same["mean"][hit] - moments["mean"][hit]) <= dc.MEAN_TOLERANCE * largest).all()
            assert (np.abs(same["m2"][hit] - moments["m2"][hit]) <= dc.M2_TOLERANCE * moments["m2"][hit]).all()


# ---- invariants ---------------------------------------------------------------------------------------------------------

def test_invariants_against_the_other_operators(hip):
    """(consistency checks, at the tolerances themselves) z = x: the extremes of agg_buckets(x) and the moments of moments_buckets(x). x - x with `y is x`:
    every cell {n, 0.0, 0.0, 0.0, 0.0}. PRODUCT: mean * count against c_xy + n * mean_x * mean_y of comoments_buckets."""
    fields = cc.main_table()
    x, y = fields[1], fields[0]
    assert np.isfinite(x.values).all() and (x.values != 0).all()
    for request, origin, width, n_buckets, t_lo, t_hi in cc.bucket_sets(*_span(fields))[1:]:
        window = dict(groups=x.groups, t_lo=t_lo, t_hi=t_hi, n_groups=4)
        states = hip.agg_buckets(x.batch, origin, width, n_buckets, **window)
        moments = hip.moments_buckets(x.batch, origin, width, n_buckets, **window)
        hit = states["count"] > 0
        largest = np.maximum(np.abs(states["min"][hit]), np.abs(states["max"][hit])).astype(np.float64)
        same = hip.derived_buckets(x.batch, y.batch, dc.expression("x_alone"), origin, width, n_buckets, **window)
        np.testing.assert_array_equal(same["count"], states["count"])
        assert same["min"][hit].tobytes() == states["min"][hit].tobytes() and same["max"][hit].tobytes() == states["max"][hit].tobytes()
        assert (np.abs(same["mean"][hit] - moments["mean"][hit]) <= dc.MEAN_TOLERANCE * largest).all(), request
        assert (np.abs(same["m2"][hit] - moments["m2"][hit]) <= dc.M2_TOLERANCE * moments["m2"][hit]).all(), request
        zero = hip.derived_buckets(x.batch, x.batch, dc.expression("difference"), origin, width, n_buckets, **window)
        expected = mdb.fresh_derived_cells(zero.shape)
        expected["count"] = states["count"]
        assert zero.tobytes() == expected.tobytes(), request
        product = hip.derived_buckets(x.batch, y.batch, dc.expression("product"), origin, width, n_buckets, **window)
        pairs = hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets, **window)
        n = pairs["count"][hit].astype(np.float64)
        total = pairs["c_xy"][hit] + n * pairs["mean_x"][hit] * pairs["mean_y"][hit]
        # sum(x * y) in f64 against the sum of the f32 products: each product is rounded once, 2^-24 of itself
        bound = n * np.maximum(np.abs(product["min"][hit]), np.abs(product["max"][hit])).astype(np.float64) * 2.0 ** -23
        assert (np.abs(product["mean"][hit] * n - total) <= bound).all(), request


def test_equal_values_have_no_variance(hip):
    steps, noisy = cc.steps_table()
    for origin, width, n_buckets in ((0, 500 * INTERVAL, 12), (0, 250 * INTERVAL, 24)):
        got = hip.derived_buckets(steps.batch, noisy.batch, mdb.derived_expr("linear", -2.0, 0.0, 1.0), origin, width, n_buckets)
        expected = dc.oracle(steps, noisy, ("linear", -2.0, 0.0, 1.0, False), None, 1, origin, width, n_buckets)
        dc.assert_cells(got, expected, f"constant {width}")
        assert (got["m2"] == 0.0).all() and (got["mean"] == got["min"].astype(np.float64)).all() and (got["min"] == got["max"]).all()


# ---- forms, determinism, shards, errors, layouts ------------------------------------------------------------------------

def _cut(field, n_pieces):
    cuts = np.linspace(0, len(field.batch), n_pieces + 1).astype(int)
    return ([field.batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])],
            [field.groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def test_forms_runs_and_shards(hip):
    fields = cc.main_table()
    x, y = fields[2], fields[0]
    expr = dc.expression("scaled_product")
    args = (-777, 1_300, 950)
    first = hip.derived_buckets(x.batch, y.batch, expr, *args, groups=x.groups, n_groups=4)
    expected = dc.oracle(x, y, "scaled_product", x.groups, 4, *args)
    dc.assert_cells(first, expected, "host form")
    assert hip.derived_buckets(x.batch, y.batch, expr, *args, groups=x.groups, n_groups=4).tobytes() == first.tobytes()
    xs, x_groups = _cut(x, 5)
    ys, _ = _cut(y, 3)
    assert hip.derived_buckets_list(xs, ys, expr, *args, groups=x_groups, n_groups=4).tobytes() == first.tobytes()
    for _ in range(2):
        on_device = hip.derived_buckets_dev(x.resident(hip), y.resident(hip), expr, *args, groups=x.groups, n_groups=4)
        assert on_device.tobytes() == first.tobytes()
    # two calls cut at a series boundary: merged in both orders, and chained through inout
    halves = []
    chained = mdb.fresh_derived_cells((4, args[2]))
    for series in ((0, 1), (2, 3)):
        x_half = mdb.SegmentBatch.concat([x.parts[k] for k in series])
        y_half = mdb.SegmentBatch.concat([y.parts[k] for k in series])
        groups = np.concatenate([np.full(len(x.parts[k]), k, dtype=np.uint32) for k in series])
        halves.append(hip.derived_buckets(x_half, y_half, expr, *args, groups=groups, n_groups=4))
        hip.derived_buckets(x_half, y_half, expr, *args, groups=groups, cells=chained)
    for merged in (mdb.derived_merge(halves[0].copy(), halves[1]), mdb.derived_merge(halves[1].copy(), halves[0]), chained):
        dc.assert_cells(merged, expected, "two calls")
        for member in ("count", "min", "max"):
            assert merged[member].tobytes() == first[member].tobytes()
    # the convenience: one bucket over the data inside the range
    whole = hip.derived(x.batch, y.batch, expr, groups=x.groups)
    lo, hi = _span(fields)
    dc.assert_cells(whole.reshape(4, 1), dc.oracle(x, y, "scaled_product", x.groups, 4, lo, hi - lo + 1, 1), "derived()")


def test_cells_that_receive_nothing_keep_their_bytes(hip):
    fields = cc.main_table()
    x, y = fields[2], fields[1]
    first, last = _span(fields)
    origin, width, n_buckets = first - 10 * 30_000, 30_000, (last - first) // 30_000 + 30
    expected = dc.oracle(x, y, "ratio", x.groups, 5, origin, width, n_buckets)   # (group 4 has no segment)
    empty = expected["count"] == 0
    assert empty[:4].any() and empty[4].all() and (~empty).any()
    cells = mdb.fresh_derived_cells((5, n_buckets))
    cells.view(np.uint8).reshape(5, n_buckets, -1)[empty] = 0xA5
    for form in ("host", "dev"):
        got = cells.copy()
        if form == "host":
            hip.derived_buckets(x.batch, y.batch, dc.expression("ratio"), origin, width, n_buckets, groups=x.groups, cells=got)
        else:
            hip.derived_buckets_dev(x.resident(hip), y.resident(hip), dc.expression("ratio"), origin, width, n_buckets, groups=x.groups, cells=got)
        assert got[empty].tobytes() == cells[empty].tobytes(), form
        got[empty] = 0
        dc.assert_cells(got, expected, form)


def test_errors_leave_the_outputs_untouched(hip):
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    first, last = _span(fields)
    cells = np.frombuffer(bytes([0xA5]) * (4 * 10 * CELL.itemsize), dtype=CELL).reshape(4, 10).copy()
    before = cells.copy()
    width = (last - first) // 10 + 1
    good = dc.expression("product")
    n = len(x.ts)
    dev_values = hip.upload_array(np.full(n, -77.0, dtype=np.float32))

    def forms(x_batch, y_batch, groups, expr=good, values=True):
        dev_a, dev_b = hip.upload_segments(x_batch), hip.upload_segments(y_batch)
        try:
            yield lambda: hip.derived_buckets(x_batch, y_batch, expr, first, width, 10, groups=groups, cells=cells)
            yield lambda: hip.derived_buckets_list([x_batch], [y_batch], expr, first, width, 10, groups=[groups], cells=cells)
            yield lambda: hip.derived_buckets_dev(dev_a, dev_b, expr, first, width, 10, groups=groups, cells=cells)
            if values:
                yield lambda: hip.derived_values(x_batch, y_batch, expr)
                yield lambda: hip.derived_values_dev(dev_a, dev_b, expr, I64_MIN, I64_MAX, None, dev_values, n)
        finally:
            dev_a.free()
            dev_b.free()

    def untouched():
        return cells.tobytes() == before.tobytes() and (hip.download_array(dev_values, n, np.float32) == -77.0).all()

    try:
        # a y with one series shortened: the message holds both row counts
        shorter = mdb.SegmentBatch.concat([y.parts[0], y.parts[1], y.parts[2], y.parts[3].slice(0, len(y.parts[3]) - 1)])
        n_short = n - int(y.rows[-1])
        for call in forms(x.batch, shorter, x.groups):
            with pytest.raises(mdb.HipError, match=rf"{n} rows.*{n_short} rows.*line up"):
                call()
            assert untouched()
        # a bad op, a bad flag, a NaN coefficient
        for expr, message in ((_abi.DerivedExprC(3, 0, 1.0, 1.0, 0.0), "op"), (_abi.DerivedExprC(0, 2, 1.0, 1.0, 0.0), "flag"),
                              (_abi.DerivedExprC(0, 0, 1.0, np.nan, 0.0), "finite")):
            for call in forms(x.batch, y.batch, x.groups, expr):
                with pytest.raises(mdb.HipError, match=message):
                    call()
                assert untouched()
        # a malformed segment in x, and one in y: a row of a model type that does not exist
        for which in ("x", "y"):
            field = x if which == "x" else y
            rows = field.batch.rows()
            rows[len(rows) // 2] = (_abi.MDB_MACAQUE_V_ID + 1,) + rows[len(rows) // 2][1:]
            broken = mdb.SegmentBatch.from_rows(rows)
            for call in forms(broken if which == "x" else x.batch, broken if which == "y" else y.batch, x.groups):
                with pytest.raises(mdb.HipError, match="model type"):
                    call()
                assert untouched()
        # a capacity too small: the message names the count
        with pytest.raises(mdb.HipError, match=rf"{n} rows.*capacity"):
            hip.derived_values_dev(x.resident(hip), y.resident(hip), good, I64_MIN, I64_MAX, None, dev_values, n - 1)
        host_values, rows = np.full(n, -77.0, dtype=np.float32), ctypes.c_uint64(99)
        seg_x, seg_y = x.batch.as_c(), y.batch.as_c()
        assert hip.lib.mdb_derived_values(hip.handle, ctypes.byref(seg_x), ctypes.byref(seg_y), ctypes.byref(good), I64_MIN, I64_MAX,
                                          None, host_values.ctypes.data, n - 1, ctypes.byref(rows)) == 1
        assert str(n).encode() in hip.lib.mdb_last_error() and (host_values == -77.0).all() and rows.value == 99 and untouched()
        # a group id out of range
        bad = x.groups.copy()
        bad[-1] = 4
        for call in forms(x.batch, y.batch, bad, values=False):
            with pytest.raises(mdb.HipError, match="group id"):
                call()
            assert untouched()
        # a scratch limit below the two columns: the message names the bytes
        limited = mdb.Context(0)
        try:
            limited.set_scratch_limit(6 * n)   # (the y column fits, the two columns do not)
            with pytest.raises(mdb.HipError, match=rf"{8 * n} bytes"):
                limited.derived_buckets(x.batch, y.batch, good, first, width, 10, groups=x.groups, cells=cells)
            assert untouched()
            limited.set_scratch_limit(0)
            got = limited.derived_buckets(x.batch, y.batch, good, first, width, 10, groups=x.groups, n_groups=4)
            assert got.tobytes() == hip.derived_buckets(x.batch, y.batch, good, first, width, 10, groups=x.groups, n_groups=4).tobytes()
        finally:
            limited.set_scratch_limit(0)
            limited.close()
    finally:
        hip.dev_free(dev_values)


def test_empty_input_succeeds_and_changes_nothing(hip):
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    first, last = _span(fields)
    rng = np.random.default_rng(10)
    cells = np.frombuffer(rng.bytes(4 * 10 * CELL.itemsize), dtype=CELL).reshape(4, 10).copy()
    cells["count"] = np.abs(cells["count"] >> 2) + 1
    before = cells.copy()
    expr = dc.expression("product")
    empty = x.batch.slice(0, 0)
    hip.derived_buckets(empty, empty, expr, 0, 100, 10, cells=cells, n_groups=4)
    hip.derived_buckets_list([], [], expr, 0, 100, 10, cells=cells, n_groups=4)
    hip.derived_buckets(x.batch, y.batch, expr, first, 1000, 10, groups=x.groups, t_lo=last + 10, t_hi=last + 1000, cells=cells)
    hip.derived_buckets(x.batch, y.batch, expr, first, 1000, 10, groups=x.groups, t_lo=first + 10, t_hi=first + 9, cells=cells)
    hip.derived_buckets_dev(x.resident(hip), y.resident(hip), expr, last + 1, 1000, 10, groups=x.groups, cells=cells)
    assert cells.tobytes() == before.tobytes()
    none = np.zeros((4, 0), dtype=CELL)
    assert hip.derived_buckets(x.batch, y.batch, expr, 0, 100, 0, groups=x.groups, cells=none).shape == (4, 0)
    for batch in (empty, x.batch):
        ts, z = hip.derived_values(batch, batch, expr, last + 10, last + 1000)
        assert len(ts) == 0 and len(z) == 0


@pytest.mark.parametrize("mode", layouts.MODES)
def test_every_layout_gives_the_same_bytes(hip, mode):
    """Every layout of tests/layouts.py through one buckets call and one values call: the bytes of the canonical layout."""
    batch, _, _ = layouts.corpus()
    other = layouts.relayout(batch, mode, 1)
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    args = (first - 5, (last - first) // 37 + 1, 40)
    expr = dc.expression("weighted_sum")
    canonical = hip.derived_buckets(batch, batch, expr, *args)
    assert int(canonical["count"].sum()) == int(ora.grid_batch(batch)[2].sum())
    assert hip.derived_buckets(other, batch, expr, *args).tobytes() == canonical.tobytes()
    assert hip.derived_buckets(batch, other, expr, *args).tobytes() == canonical.tobytes()
    ts, z = hip.derived_values(batch, batch, expr)
    for a, b in ((other, batch), (batch, other)):
        got_ts, got = hip.derived_values(a, b, expr)
        assert np.array_equal(got_ts, ts) and got.tobytes() == z.tobytes()
