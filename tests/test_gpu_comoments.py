"""Covariance and correlation of two fields on segments (mdb_comoments_buckets*): per date_bin bucket and group the
count, both means, both m2 and c_xy = sum((x - mean_x) * (y - mean_y)) of the pairs (x, y), row r of x's range grid
with row r of y's. The tables and the oracle are tests/comoments_cases.py's: every field compressed on its own under
its own error bound, the cells from the oracle's grids in exact arithmetic (math.fsum) with d = v - v[0] in f64.

Tolerances (tests/test_gpu_moments.py's, and for c_xy its Cauchy-Schwarz scale): count exact; each mean within 2^-44 of
the cell's largest |v| of that field; each m2 within 1e-5 of its reference; |c_xy - c_ref| <= 1e-5 * sqrt(m2x_ref *
m2y_ref) - a relative bound on a covariance near zero has no meaning. In a cell that holds a NaN or an infinity in a
field, that field's mean and m2 and c_xy are not finite, and nothing more is asked. Expected values never come from
the library under test, except in the tests that say they are consistency checks."""

import ctypes

import numpy as np
import pytest

import cases
import comoments_cases as cc
import datagen
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
CELL = mdb.COMOMENTS_CELL_DTYPE
EDGE_EPOCH = 1658671178037  # the first timestamp of the edge cases' epoch-scale series
PAIRS = [(a, b) for a in range(3) for b in range(3) if a != b]


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()


def _span(fields):
    return int(fields[0].ts.min()), int(fields[0].ts.max())


def _requests(fields):
    return cc.bucket_sets(*_span(fields))


def _shortened_ranges(x, y):
    """(t_hi, t_ok) of test_errors_leave_the_cells_untouched: y's last series loses its last segment; a range that ends
    on the first of the missing rows, and one that ends in front of the last series."""
    return int(y.parts[3].end_time[-2]) + INTERVAL, int(x.parts[3].start_time[0]) - 1


def test_tables_line_up_under_every_range_used():
    """With the oracle alone: count and timestamps of the rows of every field agree under every range the tests use,
    and the fields are cut into different segments."""
    main, edge = cc.main_table(), cc.edge_table()
    last = _span(main)[1]
    # (the bucket sets hold every range but those of the tests of the errors, the convenience and the empty input)
    on_the_gap, in_front = _shortened_ranges(main[0], main[1])
    cc.assert_lined_up(main, {(t_lo, t_hi) for _, _, _, _, t_lo, t_hi in _requests(main)}
                       | {(I64_MIN, on_the_gap), (I64_MIN, in_front), (last + 1, I64_MAX), (last + 10, last + 1000)})
    cc.assert_lined_up(edge, [(I64_MIN, I64_MAX), (150, 950), (EDGE_EPOCH + 100_500, EDGE_EPOCH + 300_400)])
    assert len({len(field.batch) for field in main}) == 3
    for part_lengths in zip(*[[len(part) for part in field.parts] for field in main]):
        assert len(set(part_lengths)) > 1
    lengths = main[1].rows[main[1].groups == 2], main[2].rows[main[2].groups == 3]
    assert lengths[0].mean() > 4 * 64 and lengths[1].mean() < 64 / 2   # (segments far longer / far shorter than 64 rows)
    types = set(np.concatenate([field.batch.model_type_id for field in main]).tolist())
    assert types == {mdb.MDB_PMC_MEAN_ID, mdb.MDB_SWING_ID, mdb.MDB_MACAQUE_V_ID}


@pytest.mark.parametrize("pair", PAIRS, ids=[f"x{a}_y{b}" for a, b in PAIRS])
def test_parity_with_the_points_in_exact_arithmetic(hip, pair):
    fields = cc.main_table()
    x, y = fields[pair[0]], fields[pair[1]]
    for name, origin, width, n_buckets, t_lo, t_hi in _requests(fields):
        for groups, n_groups in ((x.groups, 4), (None, 1)):
            got = hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi,
                                        n_groups=n_groups)
            cc.assert_cells(got, cc.oracle(x, y, groups, n_groups, origin, width, n_buckets, t_lo, t_hi),
                            f"x{pair[0]} y{pair[1]} {name} {n_groups} group(s)")


@pytest.mark.parametrize("pair", [(0, 1), (1, 0)], ids=["lossless_abs5", "abs5_lossless"])
def test_edge_table(hip, pair):
    """NaN, +-0, +-inf, one- and two-point segments, epoch-scale Swing: each series a group."""
    fields = cc.edge_table()
    x, y = fields[pair[0]], fields[pair[1]]
    n_groups = len(x.parts)
    special = 0
    for origin, width, n_buckets, t_lo, t_hi in ((0, 100, 40, I64_MIN, I64_MAX), (-35, 250, 24, 150, 950),
                                                 (EDGE_EPOCH - 1000, 3000, 30, I64_MIN, I64_MAX),
                                                 (EDGE_EPOCH, 50_000, 10, EDGE_EPOCH + 100_500, EDGE_EPOCH + 300_400),
                                                 (0, 1 << 40, 3, I64_MIN, I64_MAX)):
        got = hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets, groups=x.groups, t_lo=t_lo, t_hi=t_hi,
                                    n_groups=n_groups)
        expected = cc.oracle(x, y, x.groups, n_groups, origin, width, n_buckets, t_lo, t_hi)
        cc.assert_cells(got, expected, f"edge {origin} {width}")
        special += int(((expected["count"] > 0) & ~(expected["finite_x"] & expected["finite_y"])).sum())
        np.testing.assert_array_equal(got["count"], hip.agg_buckets(x.batch, origin, width, n_buckets, groups=x.groups,
                                                                    t_lo=t_lo, t_hi=t_hi, n_groups=n_groups)["count"])
    assert special > 0   # (cells with a NaN or an infinity were among them)


def test_a_field_constant_per_bucket_has_no_covariance(hip):
    """Long PMC-Mean runs against a noisy field, buckets that divide the runs: c_xy == 0.0 and the constant field's
    m2 == 0.0 exactly, whichever side it is on."""
    steps, noisy = cc.steps_table()
    assert (steps.batch.model_type_id == mdb.MDB_PMC_MEAN_ID).all() and len(steps.batch) >= 12
    for origin, width, n_buckets in ((0, 500 * INTERVAL, 12), (0, 250 * INTERVAL, 24), (0, 100 * INTERVAL, 60)):
        for x, y, constant in ((steps, noisy, "x"), (noisy, steps, "y")):
            got = hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets)
            cc.assert_cells(got, cc.oracle(x, y, None, 1, origin, width, n_buckets), f"constant {constant} {width}")
            assert (got["count"] == width // INTERVAL).all()
            assert (got["c_xy"] == 0.0).all() and (got["m2_" + constant] == 0.0).all()
            other = "y" if constant == "x" else "x"
            assert (got["m2_" + other] > 0.0).all()
            assert np.isnan(mdb.comoments_finish(got, "corr")).all()


def test_self_pair(hip):
    """comoments(x, x) with one pointer, and with two separately uploaded copies: m2_x, m2_y and c_xy of the same
    bytes, mean_x == mean_y, corr exactly 1.0 where m2 > 0."""
    fields = cc.main_table()
    first, last = _span(fields)
    for x in fields:
        for origin, width, n_buckets in ((first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2),
                                         (first, last - first + 1, 1)):
            one = hip.comoments_buckets(x.batch, x.batch, origin, width, n_buckets, groups=x.groups, n_groups=4)
            copy = mdb.SegmentBatch.from_rows(x.batch.rows())
            second = hip.upload_segments(copy)
            two = hip.comoments_buckets_dev(x.resident(hip), second, origin, width, n_buckets, groups=x.groups, n_groups=4)
            second.free()
            same = hip.comoments_buckets_dev(x.resident(hip), x.resident(hip), origin, width, n_buckets, groups=x.groups,
                                             n_groups=4)
            cc.assert_cells(one, cc.oracle(x, x, x.groups, 4, origin, width, n_buckets), f"self {width}")
            for got in (one, two, same):
                assert got.tobytes() == one.tobytes()
                assert got["m2_x"].tobytes() == got["m2_y"].tobytes() == got["c_xy"].tobytes()
                assert got["mean_x"].tobytes() == got["mean_y"].tobytes()
            corr = mdb.comoments_finish(one, "corr")
            assert (corr[one["m2_x"] > 0.0] == 1.0).all() and np.isnan(corr[one["m2_x"] == 0.0]).all()


def test_swap_exchanges_the_members(hip):
    """comoments(y, x) with y's groups: the members exchanged; both calls are held to the oracle with the same
    tolerances, so they are within twice the tolerance of each other."""
    fields = cc.main_table()
    first, last = _span(fields)
    args = (first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2)
    x, y = fields[0], fields[2]
    forward = hip.comoments_buckets(x.batch, y.batch, *args, groups=x.groups, n_groups=4)
    backward = hip.comoments_buckets(y.batch, x.batch, *args, groups=y.groups, n_groups=4)
    expected = cc.oracle(x, y, x.groups, 4, *args)
    cc.assert_cells(forward, expected, "forward")
    swapped = mdb.fresh_comoments_cells(backward.shape)
    swapped["count"] = backward["count"]
    for name, other in (("mean_x", "mean_y"), ("mean_y", "mean_x"), ("m2_x", "m2_y"), ("m2_y", "m2_x"), ("c_xy", "c_xy")):
        swapped[name] = backward[other]
    cc.assert_cells(swapped, expected, "backward, members exchanged")


def test_consistency_with_moments_buckets_and_agg_buckets(hip):
    """(a consistency check) The x-triple against moments_buckets(x), the y-triple against moments_buckets(y) within
    the moments tolerances; count equals mdb_agg_buckets' COUNT."""
    fields = cc.main_table()
    x, y = fields[1], fields[0]
    for name, origin, width, n_buckets, t_lo, t_hi in _requests(fields)[1:]:
        cells = hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets, groups=x.groups, t_lo=t_lo, t_hi=t_hi,
                                      n_groups=4)
        states = hip.agg_buckets(x.batch, origin, width, n_buckets, groups=x.groups, t_lo=t_lo, t_hi=t_hi, n_groups=4)
        np.testing.assert_array_equal(cells["count"], states["count"])
        hit = cells["count"] > 0
        for which, field in ((0, x), (1, y)):
            triple = mdb.comoments_moments(cells, which)
            # (y's points fall into the cells of x's segments' groups: the same series, so the same groups)
            moments = hip.moments_buckets(field.batch, origin, width, n_buckets, groups=field.groups, t_lo=t_lo,
                                          t_hi=t_hi, n_groups=4)
            np.testing.assert_array_equal(triple["count"], moments["count"])
            extremes = hip.agg_buckets(field.batch, origin, width, n_buckets, groups=field.groups, t_lo=t_lo, t_hi=t_hi,
                                       n_groups=4)
            largest = np.maximum(np.abs(extremes["min"][hit]), np.abs(extremes["max"][hit])).astype(np.float64)
            assert (np.abs(triple["mean"][hit] - moments["mean"][hit]) <= cc.MEAN_TOLERANCE * largest).all(), name
            assert (np.abs(triple["m2"][hit] - moments["m2"][hit]) <= cc.M2_TOLERANCE * moments["m2"][hit]).all(), name
            variance = mdb.moments_variance(triple, 1)
            assert np.isnan(variance[cells["count"] <= 1]).all()


def _cut(field, n_pieces):
    cuts = np.linspace(0, len(field.batch), n_pieces + 1).astype(int)
    return ([field.batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])],
            [field.groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def test_forms_and_runs_agree_bit_for_bit(hip):
    fields = cc.main_table()
    x, y = fields[2], fields[0]
    args = (-777, 1_300, 950)
    first = hip.comoments_buckets(x.batch, y.batch, *args, groups=x.groups, n_groups=4)
    expected = cc.oracle(x, y, x.groups, 4, *args)
    cc.assert_cells(first, expected, "host form")
    assert hip.comoments_buckets(x.batch, y.batch, *args, groups=x.groups, n_groups=4).tobytes() == first.tobytes()
    xs, x_groups = _cut(x, 5)
    ys, _ = _cut(y, 3)   # (cut at other places, and into another number of batches)
    listed = hip.comoments_buckets_list(xs, ys, *args, groups=x_groups, n_groups=4)
    assert listed.tobytes() == first.tobytes()
    for _ in range(2):
        on_device = hip.comoments_buckets_dev(x.resident(hip), y.resident(hip), *args, groups=x.groups, n_groups=4)
        assert on_device.tobytes() == first.tobytes()
    # the halves of the series folded into the same cells
    halves = mdb.fresh_comoments_cells((4, args[2]))
    for series in ((0, 1), (2, 3)):
        x_half = mdb.SegmentBatch.concat([x.parts[k] for k in series])
        y_half = mdb.SegmentBatch.concat([y.parts[k] for k in series])
        groups = np.concatenate([np.full(len(x.parts[k]), k, dtype=np.uint32) for k in series])
        hip.comoments_buckets(x_half, y_half, *args, groups=groups, cells=halves)
    cc.assert_cells(halves, expected, "two calls, two series each")


def test_slices_and_order_stay_within_the_tolerance(hip, monkeypatch):
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    first, last = _span(fields)
    args = (first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2)
    wide = (first, last - first + 1, 1)
    expected, expected_wide = cc.oracle(x, y, x.groups, 4, *args), cc.oracle(x, y, x.groups, 4, *wide)
    cc.assert_cells(hip.comoments_buckets(x.batch, y.batch, *args, groups=x.groups, n_groups=4), expected, "plain")
    monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "300")
    hip.profile_enable(True)
    hip.profile_reset()
    sliced = hip.comoments_buckets(x.batch, y.batch, *args, groups=x.groups, n_groups=4)
    launches = hip.profile()["k_comoments_partials"][0]
    hip.profile_enable(False)
    sliced_wide = hip.comoments_buckets(x.batch, y.batch, *wide, groups=x.groups, n_groups=4)
    sliced_dev = hip.comoments_buckets_dev(x.resident(hip), y.resident(hip), *args, groups=x.groups, n_groups=4)
    monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
    assert launches > 3
    cc.assert_cells(sliced, expected, "slices of 300 pairs")
    cc.assert_cells(sliced_wide, expected_wide, "slices of 300 pairs, one bucket")
    assert sliced_dev.tobytes() == sliced.tobytes()
    # the series in reversed order in both fields (the keys out of order: the sort path)
    x_back = mdb.SegmentBatch.concat(x.parts[::-1])
    y_back = mdb.SegmentBatch.concat(y.parts[::-1])
    groups_back = np.concatenate([np.full(len(x.parts[k]), k, dtype=np.uint32) for k in (3, 2, 1, 0)])
    cc.assert_cells(hip.comoments_buckets(x_back, y_back, *args, groups=groups_back, n_groups=4), expected, "reversed")


def test_runs_of_one_cell_through_every_level_of_the_reduction_tree(hip):
    """More than 64^2 pairs in one cell: x segments of 2..12 points each (chunks of that length), in one bucket and in
    two."""
    rng = np.random.default_rng(5)
    lengths = rng.integers(2, 13, 4_200)
    n = int(lengths.sum())
    timestamps = np.arange(n, dtype=np.int64) * INTERVAL
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    x = cc.Field([hip.compress_chunks(timestamps, datagen.sine_series(31, n)[1], offsets, cases.error_bounds()["rel1"])])
    y = cc.Field([hip.compress_chunks(timestamps, datagen.sine_series(32, n)[1], np.array([0, n // 3, n], dtype=np.uint64),
                                      cases.LOSSLESS)])
    assert len(x.batch) > 64 * 64 and x.rows.max() <= 12 and len(x.ts) == len(y.ts) == n < 40_000
    first, last = _span([x])
    for width, n_buckets in ((last - first + 1, 1), ((last - first) // 2 + 1, 2)):
        got = hip.comoments_buckets(x.batch, y.batch, first, width, n_buckets)
        cc.assert_cells(got, cc.oracle(x, y, None, 1, first, width, n_buckets), f"{n_buckets} bucket(s)")


def test_macaque_v_through_the_cursor_index_and_without(hip, monkeypatch):
    """Lossless MacaqueV streams of 65 536 values on the x side and on the y side: piece by piece from the cursor index
    (k_comoments_pieces), and one lane per stream with MDB_GRID_MV_INDEX=0."""
    n = 70_000
    timestamps = np.arange(n, dtype=np.int64) * INTERVAL
    offsets = np.append(np.arange(0, n, 65536), n).astype(np.uint64)
    noisy = cc.Field([hip.compress_chunks(timestamps, datagen.sine_series(21, n)[1], offsets, cases.LOSSLESS)])
    other_offsets = np.array([0, 30_000, n], dtype=np.uint64)   # (the other field is cut elsewhere)
    smooth = cc.Field([hip.compress_chunks(timestamps, datagen.sine_series(22, n)[1], other_offsets, cases.error_bounds()["abs5"])])
    assert int((noisy.batch.model_type_id == mdb.MDB_MACAQUE_V_ID).sum()) >= 2
    cc.assert_lined_up([noisy, smooth], [(I64_MIN, I64_MAX), (12_345, 6_000_000)])
    try:
        for x, y, pieces in ((noisy, smooth, True), (smooth, noisy, False)):
            for origin, width, n_buckets, t_lo, t_hi in ((0, 777 * INTERVAL, 95, I64_MIN, I64_MAX),
                                                         (13, 30 * INTERVAL, 2_400, 12_345, 6_000_000)):
                expected = cc.oracle(x, y, None, 1, origin, width, n_buckets, t_lo, t_hi)
                hip.profile_enable(True)
                hip.profile_reset()
                got = hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets, t_lo=t_lo, t_hi=t_hi)
                kernels = hip.profile()
                assert ("k_comoments_pieces" in kernels or not pieces) and "k_comoments_partials" in kernels, sorted(kernels)
                cc.assert_cells(got, expected, f"index {width} pieces on x: {pieces}")
                on_device = hip.comoments_buckets_dev(x.resident(hip), y.resident(hip), origin, width, n_buckets,
                                                      t_lo=t_lo, t_hi=t_hi)
                assert on_device.tobytes() == got.tobytes()
                monkeypatch.setenv("MDB_GRID_MV_INDEX", "0")
                hip.profile_reset()
                serial = hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets, t_lo=t_lo, t_hi=t_hi)
                kernels = hip.profile()
                monkeypatch.delenv("MDB_GRID_MV_INDEX")
                assert "k_comoments_pieces" not in kernels and "k_comoments_partials" in kernels, sorted(kernels)
                cc.assert_cells(serial, expected, f"no index {width}")
                np.testing.assert_array_equal(serial["count"], got["count"])
    finally:
        hip.profile_enable(False)
        noisy.free()
        smooth.free()


def test_resident_batches_give_the_same_bytes_after_other_operators(hip):
    fields = cc.main_table()
    x, y = fields[1], fields[2]
    dev_x, dev_y = x.resident(hip), y.resident(hip)
    first, last = _span(fields)
    args = (first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2)
    t_lo, t_hi = first + 7_777, last - 12_321
    call = lambda: hip.comoments_buckets_dev(dev_x, dev_y, *args, groups=x.groups, t_lo=t_lo, t_hi=t_hi, n_groups=4)
    before = call()
    cc.assert_cells(before, cc.oracle(x, y, x.groups, 4, *args, t_lo, t_hi), "resident")
    assert call().tobytes() == before.tobytes()
    words = mdb.mask_words(len(x.ts))
    mask = hip.dev_alloc(8 * max(words, 1))
    try:
        for dev in (dev_x, dev_y):
            hip.grid_resident(dev)
            hip.grid_resident(dev, (t_lo, t_hi))
            hip.moments_buckets_dev(dev, *args, t_lo=t_lo, t_hi=t_hi)
            hip.mask_filter_dev(dev, mdb.value_filter(lo=120.0, t_lo=t_lo, t_hi=t_hi), mask, words)
            assert call().tobytes() == before.tobytes()
    finally:
        hip.dev_free(mask)


def test_cells_that_receive_nothing_keep_their_bytes(hip):
    fields = cc.main_table()
    x, y = fields[2], fields[1]
    first, last = _span(fields)
    origin, width, n_buckets = first - 10 * 30_000, 30_000, (last - first) // 30_000 + 30
    expected = cc.oracle(x, y, x.groups, 5, origin, width, n_buckets)   # (group 4 has no segment)
    empty = expected["count"] == 0
    assert empty[:4].any() and empty[4].all() and (~empty).any()
    cells = mdb.fresh_comoments_cells((5, n_buckets))
    cells.view(np.uint8).reshape(5, n_buckets, -1)[empty] = 0xA5
    pattern = cells.copy()
    for form in ("host", "dev"):
        got = cells.copy()
        if form == "host":
            hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets, groups=x.groups, cells=got)
        else:
            hip.comoments_buckets_dev(x.resident(hip), y.resident(hip), origin, width, n_buckets, groups=x.groups, cells=got)
        assert got[empty].tobytes() == pattern[empty].tobytes(), form
        filled = got.copy()
        filled[empty] = 0
        cc.assert_cells(filled, expected, form)
    # a merge into cells that are not fresh is comoments_merge of the two results
    args = (origin, width, n_buckets)
    half = len(x.parts[0]) + len(x.parts[1])
    y_half = len(y.parts[0]) + len(y.parts[1])
    one = hip.comoments_buckets(x.batch.slice(0, half), y.batch.slice(0, y_half), *args, groups=x.groups[:half], n_groups=5)
    other = hip.comoments_buckets(x.batch.slice(half, len(x.batch)), y.batch.slice(y_half, len(y.batch)), *args,
                                  groups=x.groups[half:], n_groups=5)
    merged = mdb.comoments_merge(one.copy(), other)
    into = hip.comoments_buckets(x.batch.slice(half, len(x.batch)), y.batch.slice(y_half, len(y.batch)), *args,
                                 groups=x.groups[half:], cells=one.copy())
    cc.assert_cells(merged, expected, "comoments_merge of two calls")
    cc.assert_cells(into, expected, "the second call into the first one's cells")


def test_the_ungrouped_in_time_convenience_and_the_statistics(hip):
    """Context.comoments is one bucket over the data inside the range; comoments_finish gives numpy's statistics."""
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    first, last = _span(fields)
    for t_lo, t_hi in ((None, None), (first + 7_777, last - 12_321), (last + 1, None)):
        cells = hip.comoments(x.batch, y.batch, t_lo, t_hi, groups=x.groups)
        assert cells.shape == (4,)
        lo, hi = I64_MIN if t_lo is None else t_lo, I64_MAX if t_hi is None else t_hi
        xv, yv = x.values[x.in_range(lo, hi)].astype(np.float64), y.values[y.in_range(lo, hi)].astype(np.float64)
        series = x.groups[x.segment[x.in_range(lo, hi)]]
        for g in range(4):
            px, py = xv[series == g], yv[series == g]
            assert cells["count"][g] == len(px)
            if len(px) < 2:
                assert np.isnan(mdb.comoments_finish(cells, "corr")[g])
                continue
            slope, intercept = np.polyfit(px, py, 1)
            corr = np.corrcoef(px, py)[0, 1]
            for kind, value in (("covar_pop", np.cov(px, py, ddof=0)[0, 1]), ("covar_samp", np.cov(px, py, ddof=1)[0, 1]),
                                ("corr", corr), ("regr_slope", slope), ("regr_intercept", intercept), ("regr_r2", corr * corr)):
                got = mdb.comoments_finish(cells, kind)[g]
                assert abs(got - value) <= 1e-7 * max(abs(value), 1.0), (kind, got, value)


def test_errors_leave_the_cells_untouched(hip):
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    first, last = _span(fields)
    size = CELL.itemsize
    cells = np.frombuffer(bytes([0xA5]) * (4 * 10 * size), dtype=CELL).reshape(4, 10).copy()
    before = cells.copy()
    width = (last - first) // 10 + 1
    dev_x, dev_y = x.resident(hip), y.resident(hip)

    def forms(x_batch, y_batch, groups, **more):
        dev_a, dev_b = hip.upload_segments(x_batch), hip.upload_segments(y_batch)
        try:
            yield lambda: hip.comoments_buckets(x_batch, y_batch, first, width, 10, groups=groups, cells=cells, **more)
            yield lambda: hip.comoments_buckets_list([x_batch], [y_batch], first, width, 10, groups=[groups], cells=cells, **more)
            yield lambda: hip.comoments_buckets_dev(dev_a, dev_b, first, width, 10, groups=groups, cells=cells, **more)
        finally:
            dev_a.free()
            dev_b.free()

    # a y with one series shortened: the message holds both row counts
    shorter = mdb.SegmentBatch.concat([y.parts[0], y.parts[1], y.parts[2], y.parts[3].slice(0, len(y.parts[3]) - 1)])
    n_x, n_short = len(x.ts), len(x.ts) - int(y.rows[-1])
    for a, b, counts in ((x.batch, shorter, (n_x, n_short)), (shorter, x.batch, (n_short, n_x))):
        groups = x.groups if a is x.batch else np.zeros(len(shorter), dtype=np.uint32)
        for call in forms(a, b, groups):
            with pytest.raises(mdb.HipError, match=rf"{counts[0]} rows.*{counts[1]} rows.*line up"):
                call()
            assert cells.tobytes() == before.tobytes()
    # a range under which the counts differ: it ends on the first of the missing rows
    t_hi, t_ok = _shortened_ranges(x, y)
    assert t_hi == int(shorter.end_time[-1]) + INTERVAL
    assert int(x.in_range(I64_MIN, t_hi).sum()) != int((cc.Field([shorter]).ts <= t_hi).sum())
    for call in forms(x.batch, shorter, x.groups, t_hi=t_hi):
        with pytest.raises(mdb.HipError, match="line up"):
            call()
        assert cells.tobytes() == before.tobytes()
    # (and a range that ends before the shortened part lines up again)
    ok = hip.comoments_buckets(x.batch, shorter, first, width, 10, groups=x.groups, t_hi=t_ok, n_groups=4)
    cc.assert_cells(ok, cc.oracle(x, y, x.groups, 4, first, width, 10, I64_MIN, t_ok), "a range in front of the missing rows")
    # a group id out of range
    bad = x.groups.copy()
    bad[-1] = 4
    for call in forms(x.batch, y.batch, bad, t_hi=t_ok):
        with pytest.raises(mdb.HipError, match="group id"):
            call()
        assert cells.tobytes() == before.tobytes()
    # a malformed segment in x, and one in y: a row of a model type that does not exist
    for which in ("x", "y"):
        field = x if which == "x" else y
        rows = field.batch.rows()
        rows[len(rows) // 2] = (_abi.MDB_MACAQUE_V_ID + 1,) + rows[len(rows) // 2][1:]
        broken = mdb.SegmentBatch.from_rows(rows)
        for call in forms(broken if which == "x" else x.batch, broken if which == "y" else y.batch, x.groups):
            with pytest.raises(mdb.HipError, match="model type"):
                call()
            assert cells.tobytes() == before.tobytes()
    # a scratch limit below the y column: the message names the bytes
    limited = mdb.Context(0)
    try:
        limited.set_scratch_limit(4096)
        needed = 4 * len(x.ts)
        with pytest.raises(mdb.HipError, match=rf"{needed} bytes"):
            limited.comoments_buckets(x.batch, y.batch, first, width, 10, groups=x.groups, cells=cells)
        assert cells.tobytes() == before.tobytes()
        limited.set_scratch_limit(0)
        got = limited.comoments_buckets(x.batch, y.batch, first, width, 10, groups=x.groups, n_groups=4)
        assert got.tobytes() == hip.comoments_buckets(x.batch, y.batch, first, width, 10, groups=x.groups, n_groups=4).tobytes()
    finally:
        limited.set_scratch_limit(0)
        limited.close()
    # requests, NULL arguments
    seg_x, seg_y = x.batch.as_c(), y.batch.as_c()
    data = cells.ctypes.data_as(ctypes.c_void_p)
    for origin, w, n_groups, which_mask, message in ((0, 100, 4, 1, b"which_mask"), (0, 0, 4, 0, b"width"),
                                                     (0, -5, 4, 0, b"width"), (0, 100, 0, 0, b"n_groups")):
        request = _abi.BucketRequestC(origin, w, 10, I64_MIN, I64_MAX, n_groups, which_mask)
        assert hip.lib.mdb_comoments_buckets(hip.handle, ctypes.byref(seg_x), ctypes.byref(seg_y), None, ctypes.byref(request), data) == 1
        assert message in hip.lib.mdb_last_error()
        assert hip.lib.mdb_comoments_buckets_dev(hip.handle, ctypes.byref(dev_x.seg), ctypes.byref(dev_y.seg), None,
                                                 ctypes.byref(request), data) == 1
        assert message in hip.lib.mdb_last_error()
    request = _abi.BucketRequestC(0, 100, 10, I64_MIN, I64_MAX, 4, 0)
    assert hip.lib.mdb_comoments_buckets(hip.handle, ctypes.byref(seg_x), None, None, ctypes.byref(request), data) == 1
    assert b"NULL" in hip.lib.mdb_last_error()
    assert hip.lib.mdb_comoments_buckets_dev(hip.handle, ctypes.byref(dev_x.seg), None, None, ctypes.byref(request), data) == 1
    assert b"NULL" in hip.lib.mdb_last_error()
    assert hip.lib.mdb_comoments_buckets(hip.handle, None, ctypes.byref(seg_y), None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_comoments_buckets(None, ctypes.byref(seg_x), ctypes.byref(seg_y), None, ctypes.byref(request), data) == 1
    assert hip.lib.mdb_comoments_buckets(hip.handle, ctypes.byref(seg_x), ctypes.byref(seg_y), None, None, data) == 1
    assert hip.lib.mdb_comoments_buckets(hip.handle, ctypes.byref(seg_x), ctypes.byref(seg_y), None, ctypes.byref(request), None) == 1
    assert cells.tobytes() == before.tobytes()


def test_empty_input_succeeds_and_changes_nothing(hip):
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    first, last = _span(fields)
    rng = np.random.default_rng(10)
    cells = np.frombuffer(rng.bytes(4 * 10 * CELL.itemsize), dtype=CELL).reshape(4, 10).copy()
    cells["count"] = np.abs(cells["count"] >> 2) + 1
    before = cells.copy()
    empty = x.batch.slice(0, 0)
    hip.comoments_buckets(empty, empty, 0, 100, 10, cells=cells, n_groups=4)
    hip.comoments_buckets(empty, y.batch.slice(0, 0), 0, 100, 10, cells=cells, n_groups=4)
    hip.comoments_buckets_list([], [], 0, 100, 10, cells=cells, n_groups=4)
    # an empty range, and buckets the data does not reach
    hip.comoments_buckets(x.batch, y.batch, first, 1000, 10, groups=x.groups, t_lo=last + 10, t_hi=last + 1000, cells=cells)
    hip.comoments_buckets_dev(x.resident(hip), y.resident(hip), last + 1, 1000, 10, groups=x.groups, cells=cells)
    assert cells.tobytes() == before.tobytes()
    none = np.zeros((4, 0), dtype=CELL)
    assert hip.comoments_buckets(x.batch, y.batch, 0, 100, 0, groups=x.groups, cells=none).shape == (4, 0)
    assert hip.comoments_buckets_dev(x.resident(hip), y.resident(hip), 0, 100, 0, groups=x.groups, cells=none).shape == (4, 0)
