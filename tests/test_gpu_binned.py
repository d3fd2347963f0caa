"""The moments of one field per value cell of another on segments (mdb_binned_buckets*): per date_bin bucket, group and
cell of x the count, the mean and m2 of the y values of the pairs whose x value falls in the cell. The tables are
tests/comoments_cases.py's, the oracle tests/binned_cases.py's: the oracle's grids of x and y, the pairs and buckets of
comoments_cases.oracle, the cell of x by totalOrder key, and per cell the mean and m2 of y in exact arithmetic.

Tolerances (tests/test_gpu_moments.py's): count exact; mean within 2^-44 of the cell's largest |y|; m2 within 1e-5 of its
reference and not negative. In a cell that holds a NaN or an infinity of y neither mean nor m2 is finite, and nothing
more is asked. Expected values never come from the library under test, except in the tests that say they are
consistency checks."""

import ctypes

import numpy as np
import pytest

import binned_cases as bc
import comoments_cases as cc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
CELL = mdb.MOMENTS_CELL_DTYPE
PAIRS = [(a, b) for a in range(3) for b in range(3) if a != b]
EDGE_LIST = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], dtype=np.float32)


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()
    print(f"largest errors of the module: mean error / max|y| {bc.WORST['mean']:.3g}, m2 error / m2 {bc.WORST['m2']:.3g}")


def _span(fields):
    return int(fields[0].ts.min()), int(fields[0].ts.max())


def _wide(fields):
    first, last = _span(fields)
    return first, last - first + 1, 1


def _narrow(fields):
    first, last = _span(fields)
    return first - 40, 13 * INTERVAL, (last - first) // (13 * INTERVAL) + 2


@pytest.mark.parametrize("pair", PAIRS, ids=[f"x{a}_y{b}" for a, b in PAIRS])
def test_parity_with_the_points_in_exact_arithmetic(hip, pair):
    fields = cc.main_table()
    x, y = fields[pair[0]], fields[pair[1]]
    for n_edges in (1, 8, 63):
        edges = bc.quantile_edges(x.values, n_edges)
        # from the oracle alone: one bucket leaves no cell empty, and the runs are neither the segments nor the rows
        whole = bc.oracle(x, y, edges, None, 1, *_wide(fields))
        assert (whole["count"] > 0).all() and len(x.batch) < whole["runs"] < len(x.ts), (n_edges, whole["runs"])
        for name, origin, width, n_buckets, t_lo, t_hi in cc.bucket_sets(*_span(fields)):
            for groups, n_groups in ((x.groups, 4), (None, 1)):
                got = hip.binned_buckets(x.batch, y.batch, edges, origin, width, n_buckets, groups=groups, t_lo=t_lo,
                                         t_hi=t_hi, n_groups=n_groups)
                expected = bc.oracle(x, y, edges, groups, n_groups, origin, width, n_buckets, t_lo, t_hi)
                bc.assert_cells(got, expected, f"x{pair[0]} y{pair[1]} {len(edges)} edges {name} {n_groups} group(s)")


@pytest.mark.parametrize("pair", [(0, 1), (1, 0)], ids=["lossless_abs5", "abs5_lossless"])
def test_edge_table(hip, pair):
    """NaN, +-0, +-inf, one- and two-point segments, epoch-scale Swing, each series a group, under the edges -inf, -1,
    -0.0, +0.0, 1, +inf. With the lossless field as x every cell but the lowest is populated (under absolute 5 the
    cell [+0.0, 1) stays empty as well)."""
    fields = cc.edge_table()
    x, y = fields[pair[0]], fields[pair[1]]
    n_groups = len(x.parts)
    populated = bc.oracle(x, y, EDGE_LIST, None, 1, 0, 1 << 40, 3)["count"].sum(axis=(0, 1)) > 0
    assert not populated[0] and populated[[1, 2, 4, 5, 6]].all() and (populated[3] or pair[0] == 1)
    special = 0
    epoch = 1658671178037   # the first timestamp of the edge cases' epoch-scale series
    for origin, width, n_buckets, t_lo, t_hi in ((0, 100, 40, I64_MIN, I64_MAX), (-35, 250, 24, 150, 950),
                                                 (epoch - 1000, 3000, 30, I64_MIN, I64_MAX),
                                                 (epoch, 50_000, 10, epoch + 100_500, epoch + 300_400),
                                                 (0, 1 << 40, 3, I64_MIN, I64_MAX)):
        got = hip.binned_buckets(x.batch, y.batch, EDGE_LIST, origin, width, n_buckets, groups=x.groups, t_lo=t_lo,
                                 t_hi=t_hi, n_groups=n_groups)
        expected = bc.oracle(x, y, EDGE_LIST, x.groups, n_groups, origin, width, n_buckets, t_lo, t_hi)
        bc.assert_cells(got, expected, f"edge {origin} {width}")
        special += int(((expected["count"] > 0) & ~expected["finite"]).sum())
        counts = hip.hist_buckets(x.batch, EDGE_LIST, origin, width, n_buckets, groups=x.groups, t_lo=t_lo, t_hi=t_hi,
                                  n_groups=n_groups)
        np.testing.assert_array_equal(got["count"], counts.astype(np.int64))
    assert special > 0   # (cells with a NaN or an infinity of y were among them)


def _fold_over_cells(cells):
    folded = np.ascontiguousarray(cells[:, :, 0])
    for c in range(1, cells.shape[2]):
        mdb.moments_merge(folded, np.ascontiguousarray(cells[:, :, c]))
    return folded


def test_the_three_invariants(hip):
    """(a consistency check) count against hist_buckets(x), its sum over the cells against agg_buckets' COUNT, and the
    cells merged over c against the y moments of comoments_buckets(x, y) within the moments tolerances."""
    fields = cc.main_table()
    for a, b in ((0, 1), (1, 2), (2, 0)):
        x, y = fields[a], fields[b]
        edges = bc.quantile_edges(x.values, 8)
        for name, origin, width, n_buckets, t_lo, t_hi in cc.bucket_sets(*_span(fields))[1:]:
            more = dict(groups=x.groups, t_lo=t_lo, t_hi=t_hi, n_groups=4)
            cells = hip.binned_buckets(x.batch, y.batch, edges, origin, width, n_buckets, **more)
            counts = hip.hist_buckets(x.batch, edges, origin, width, n_buckets, **more)
            np.testing.assert_array_equal(cells["count"], counts.astype(np.int64), err_msg=name)
            states = hip.agg_buckets(x.batch, origin, width, n_buckets, **more)
            np.testing.assert_array_equal(cells["count"].sum(axis=2), states["count"], err_msg=name)
            pairs = mdb.comoments_moments(hip.comoments_buckets(x.batch, y.batch, origin, width, n_buckets, **more), "y")
            folded = _fold_over_cells(cells)
            np.testing.assert_array_equal(folded["count"], pairs["count"], err_msg=name)
            hit = pairs["count"] > 0
            largest = bc.oracle(x, y, edges, x.groups, 4, origin, width, n_buckets, t_lo, t_hi)["largest"].max(axis=2)
            assert (np.abs(folded["mean"][hit] - pairs["mean"][hit]) <= bc.MEAN_TOLERANCE * largest[hit]).all(), name
            assert (np.abs(folded["m2"][hit] - pairs["m2"][hit]) <= bc.M2_TOLERANCE * pairs["m2"][hit]).all(), name


def test_a_y_constant_per_cell_has_no_variance(hip):
    """Levels held for 500 points against a noisy x, buckets of 500 points: in every populated cell m2 == 0.0 and the
    mean is the level, exactly."""
    steps, noisy = cc.steps_table()
    assert (steps.batch.model_type_id == mdb.MDB_PMC_MEAN_ID).all() and len(steps.batch) >= 12
    edges = bc.quantile_edges(noisy.values, 3)
    got = hip.binned_buckets(noisy.batch, steps.batch, edges, 0, 500 * INTERVAL, 12)
    expected = bc.oracle(noisy, steps, edges, None, 1, 0, 500 * INTERVAL, 12)
    bc.assert_cells(got, expected, "constant y per bucket")
    assert (expected["count"] > 0).all() and expected["runs"] > 12 * 4 * 20
    levels = steps.values[::500].astype(np.float64)
    assert len(levels) == 12
    assert (got["m2"] == 0.0).all() and (got["mean"][0] == levels[:, None]).all()
    assert (mdb.moments_variance(got, 0) == 0.0).all()


def test_many_runs_of_one_cell_through_the_levels_of_the_reduction_tree(hip):
    """One edge at the median of a noisy x: a run every other point. Tiled until a cell receives more than 4 096 runs,
    in one bucket, so that levels 1 and 2 of the tree fold one key."""
    steps, noisy = cc.steps_table()
    copies = np.tile(np.arange(len(noisy.batch)), 3)
    x, y = cc.Field([noisy.batch.take(copies)]), cc.Field([steps.batch.take(np.tile(np.arange(len(steps.batch)), 3))])
    edges = bc.quantile_edges(noisy.values, 1)
    first, last = _span([x])
    expected = bc.oracle(x, y, edges, None, 1, first, last - first + 1, 1)
    assert (expected["cell_runs"] > 4096).all() and expected["cell_runs"].sum() == expected["runs"]
    got = hip.binned_buckets(x.batch, y.batch, edges, first, last - first + 1, 1)
    bc.assert_cells(got, expected, "many runs in one cell")
    try:
        on_device = hip.binned_buckets_dev(x.resident(hip), y.resident(hip), edges, first, last - first + 1, 1)
        assert on_device.tobytes() == got.tobytes()
    finally:
        x.free()
        y.free()


def test_x_paired_with_itself(hip):
    """binned(x, x): the mean of every cell lies within the cell's edges, m2 passes the tolerance."""
    fields = cc.main_table()
    for x in fields:
        edges = bc.quantile_edges(x.values, 8)
        for args in (_wide(fields), _narrow(fields)):
            got = hip.binned_buckets(x.batch, x.batch, edges, *args, groups=x.groups, n_groups=4)
            bc.assert_cells(got, bc.oracle(x, x, edges, x.groups, 4, *args), f"self {args[1]}")
            lower = np.concatenate([[-np.inf], edges.astype(np.float64)])
            upper = np.concatenate([edges.astype(np.float64), [np.inf]])
            hit = got["count"] > 0
            assert (got["mean"] >= lower)[hit].all() and (got["mean"] <= upper)[hit].all()
            assert (got["mean"] < upper)[hit & (got["m2"] > 0.0)].all()


def _cut(field, n_pieces):
    cuts = np.linspace(0, len(field.batch), n_pieces + 1).astype(int)
    return ([field.batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])],
            [field.groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def test_forms_and_runs_agree_bit_for_bit(hip):
    fields = cc.main_table()
    x, y = fields[2], fields[0]
    edges = bc.quantile_edges(x.values, 8)
    args = (-777, 1_300, 950)
    first = hip.binned_buckets(x.batch, y.batch, edges, *args, groups=x.groups, n_groups=4)
    bc.assert_cells(first, bc.oracle(x, y, edges, x.groups, 4, *args), "host form")
    assert hip.binned_buckets(x.batch, y.batch, edges, *args, groups=x.groups, n_groups=4).tobytes() == first.tobytes()
    xs, x_groups = _cut(x, 5)
    ys, _ = _cut(y, 3)   # (cut at other places, and into another number of batches)
    for _ in range(2):
        listed = hip.binned_buckets_list(xs, ys, edges, *args, groups=x_groups, n_groups=4)
        assert listed.tobytes() == first.tobytes()
        on_device = hip.binned_buckets_dev(x.resident(hip), y.resident(hip), edges, *args, groups=x.groups, n_groups=4)
        assert on_device.tobytes() == first.tobytes()
    power_curve = hip.binned(x.batch, y.batch, edges, groups=x.groups)
    assert power_curve.shape == (4, len(edges) + 1)
    bc.assert_cells(power_curve.reshape(4, 1, -1), bc.oracle(x, y, edges, x.groups, 4, *_wide(fields)), "binned()")


def test_slices_order_and_cut_batches_stay_within_the_tolerance(hip, monkeypatch):
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    edges = bc.quantile_edges(x.values, 8)
    args, wide = _narrow(fields), _wide(fields)
    expected, expected_wide = bc.oracle(x, y, edges, x.groups, 4, *args), bc.oracle(x, y, edges, x.groups, 4, *wide)
    plain = hip.binned_buckets(x.batch, y.batch, edges, *args, groups=x.groups, n_groups=4)
    bc.assert_cells(plain, expected, "plain")
    monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "1000")
    hip.profile_enable(True)
    hip.profile_reset()
    sliced = hip.binned_buckets(x.batch, y.batch, edges, *args, groups=x.groups, n_groups=4)
    launches = hip.profile()["k_binned_partials"][0]
    hip.profile_enable(False)
    sliced_wide = hip.binned_buckets(x.batch, y.batch, edges, *wide, groups=x.groups, n_groups=4)
    sliced_dev = hip.binned_buckets_dev(x.resident(hip), y.resident(hip), edges, *args, groups=x.groups, n_groups=4)
    monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
    assert launches > 3 and expected["runs"] > 3000
    bc.assert_cells(sliced, expected, "slices of 1000 runs")
    bc.assert_cells(sliced_wide, expected_wide, "slices of 1000 runs, one bucket")
    assert sliced_dev.tobytes() == sliced.tobytes()
    np.testing.assert_array_equal(sliced["count"], plain["count"])
    # one segment with more runs than a slice holds is a slice of its own
    steps, noisy = cc.steps_table()
    median = bc.quantile_edges(noisy.values, 1)
    alone = bc.oracle(noisy, steps, median, None, 1, 0, 6_000 * INTERVAL, 1)
    assert len(noisy.batch) == 1 and alone["runs"] > 2 * 1000
    monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "1000")
    bc.assert_cells(hip.binned_buckets(noisy.batch, steps.batch, median, 0, 6_000 * INTERVAL, 1), alone, "one long segment")
    monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")
    # the series in reversed order in both fields (the keys out of order: the sort path)
    x_back = mdb.SegmentBatch.concat(x.parts[::-1])
    y_back = mdb.SegmentBatch.concat(y.parts[::-1])
    groups_back = np.concatenate([np.full(len(x.parts[k]), k, dtype=np.uint32) for k in (3, 2, 1, 0)])
    bc.assert_cells(hip.binned_buckets(x_back, y_back, edges, *args, groups=groups_back, n_groups=4), expected, "reversed")
    # the halves of the series folded into the same cells by two calls
    halves = mdb.fresh_moments_cells((4, args[2], len(edges) + 1))
    for series in ((0, 1), (2, 3)):
        x_half = mdb.SegmentBatch.concat([x.parts[k] for k in series])
        y_half = mdb.SegmentBatch.concat([y.parts[k] for k in series])
        groups = np.concatenate([np.full(len(x.parts[k]), k, dtype=np.uint32) for k in series])
        hip.binned_buckets(x_half, y_half, edges, *args, groups=groups, cells=halves)
    bc.assert_cells(halves, expected, "two calls, two series each")


def test_resident_batches_give_the_same_bytes_between_other_operators(hip):
    fields = cc.main_table()
    x, y = fields[1], fields[2]
    dev_x, dev_y = x.resident(hip), y.resident(hip)
    edges = bc.quantile_edges(x.values, 8)
    args = _narrow(fields)
    first, last = _span(fields)
    more = dict(groups=x.groups, t_lo=first + 7_777, t_hi=last - 12_321, n_groups=4)
    binned = lambda: hip.binned_buckets_dev(dev_x, dev_y, edges, *args, **more)
    others = (lambda: hip.comoments_buckets_dev(dev_x, dev_y, *args, **more),
              lambda: hip.hist_buckets_dev(dev_x, edges, *args, **more),
              lambda: hip.moments_buckets_dev(dev_x, *args, **more),
              lambda: hip.moments_buckets_dev(dev_y, *args, groups=y.groups, t_lo=more["t_lo"], t_hi=more["t_hi"], n_groups=4))
    before = binned()
    bc.assert_cells(before, bc.oracle(x, y, edges, x.groups, 4, *args, more["t_lo"], more["t_hi"]), "resident")
    assert binned().tobytes() == before.tobytes()
    for other in others:
        alone = other()
        assert binned().tobytes() == before.tobytes()
        assert other().tobytes() == alone.tobytes()
        assert binned().tobytes() == before.tobytes()


def test_cells_that_receive_nothing_keep_their_bytes(hip):
    fields = cc.main_table()
    x, y = fields[2], fields[1]
    edges = bc.quantile_edges(x.values, 8)
    first, last = _span(fields)
    origin, width, n_buckets = first - 10 * 30_000, 30_000, (last - first) // 30_000 + 30
    expected = bc.oracle(x, y, edges, x.groups, 5, origin, width, n_buckets)   # (group 4 has no segment)
    empty = expected["count"] == 0
    assert empty[:4].any() and empty[4].all() and (~empty).any()
    shape = (5, n_buckets, len(edges) + 1)
    stale = np.frombuffer(bytes([0xA5]) * (int(np.prod(shape)) * CELL.itemsize), dtype=CELL).reshape(shape).copy()
    stale["count"] = 0
    rng = np.random.default_rng(12)
    full = np.frombuffer(rng.bytes(int(np.prod(shape)) * CELL.itemsize), dtype=CELL).reshape(shape).copy()
    full["count"] = np.abs(full["count"] >> 2) + 1
    for start, name in ((stale, "stale"), (full, "random")):
        for form in ("host", "dev"):
            got = start.copy()
            if form == "host":
                hip.binned_buckets(x.batch, y.batch, edges, origin, width, n_buckets, groups=x.groups, cells=got)
            else:
                hip.binned_buckets_dev(x.resident(hip), y.resident(hip), edges, origin, width, n_buckets, groups=x.groups,
                                       cells=got)
            assert got[empty].tobytes() == start[empty].tobytes(), (name, form)
            if name == "stale":   # (count 0: no other member is read - the cells that received pairs are the call's own)
                filled = got.copy()
                filled[empty] = 0
                bc.assert_cells(filled, expected, f"{name} {form}")
            else:
                np.testing.assert_array_equal(got["count"][~empty], start["count"][~empty] + expected["count"][~empty])


def test_errors_leave_the_cells_untouched(hip):
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    first, last = _span(fields)
    edges = bc.quantile_edges(x.values, 3)
    shape = (4, 10, len(edges) + 1)
    cells = np.frombuffer(bytes([0xA5]) * (int(np.prod(shape)) * CELL.itemsize), dtype=CELL).reshape(shape).copy()
    before = cells.copy()
    width = (last - first) // 10 + 1

    def forms(x_batch, y_batch, groups, edge_list=edges, target=cells, **more):
        dev_a, dev_b = hip.upload_segments(x_batch), hip.upload_segments(y_batch)
        try:
            yield lambda: hip.binned_buckets(x_batch, y_batch, edge_list, first, width, 10, groups=groups, cells=target, **more)
            yield lambda: hip.binned_buckets_list([x_batch], [y_batch], edge_list, first, width, 10, groups=[groups],
                                                  cells=target, **more)
            yield lambda: hip.binned_buckets_dev(dev_a, dev_b, edge_list, first, width, 10, groups=groups, cells=target, **more)
        finally:
            dev_a.free()
            dev_b.free()

    # a y with one series shortened: the message holds both row counts
    shorter = mdb.SegmentBatch.concat([y.parts[0], y.parts[1], y.parts[2], y.parts[3].slice(0, len(y.parts[3]) - 1)])
    n_x, n_short = len(x.ts), len(x.ts) - int(y.rows[-1])
    for call in forms(x.batch, shorter, x.groups):
        with pytest.raises(mdb.HipError, match=rf"{n_x} rows.*{n_short} rows.*line up"):
            call()
        assert cells.tobytes() == before.tobytes()
    # a group id out of range on a row the range does not reach
    t_ok = int(x.parts[3].start_time[0]) - 1
    bad = x.groups.copy()
    bad[-1] = 4
    assert int(x.batch.start_time[-1]) > t_ok
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
    # edge lists: not increasing, -0.0 after +0.0, none, too many
    for bad_edges, message in ((np.array([1.0, 1.0], dtype=np.float32), "strictly increasing"),
                               (np.array([2.0, 1.0], dtype=np.float32), "strictly increasing"),
                               (np.array([0.0, -0.0], dtype=np.float32), "strictly increasing"),
                               (np.zeros(0, dtype=np.float32), "n_edges"),
                               (np.arange(4096, dtype=np.float32), "n_edges")):
        target = np.frombuffer(bytes([0xA5]) * (4 * 10 * (len(bad_edges) + 1) * CELL.itemsize), dtype=CELL)
        target = target.reshape(4, 10, len(bad_edges) + 1).copy()
        untouched = target.copy()
        for call in forms(x.batch, y.batch, x.groups, edge_list=bad_edges, target=target):
            with pytest.raises(mdb.HipError, match=message):
                call()
            assert target.tobytes() == untouched.tobytes()
    # a scratch limit below the y column: the message names the bytes
    limited = mdb.Context(0)
    try:
        limited.set_scratch_limit(4096)
        with pytest.raises(mdb.HipError, match=rf"{4 * len(x.ts)} bytes"):
            limited.binned_buckets(x.batch, y.batch, edges, first, width, 10, groups=x.groups, cells=cells)
        assert cells.tobytes() == before.tobytes()
        limited.set_scratch_limit(0)
        got = limited.binned_buckets(x.batch, y.batch, edges, first, width, 10, groups=x.groups, n_groups=4)
        assert got.tobytes() == hip.binned_buckets(x.batch, y.batch, edges, first, width, 10, groups=x.groups, n_groups=4).tobytes()
    finally:
        limited.set_scratch_limit(0)
        limited.close()
    # requests and NULL arguments
    seg_x, seg_y = x.batch.as_c(), y.batch.as_c()
    data, edge_data = cells.ctypes.data_as(ctypes.c_void_p), edges.ctypes.data_as(ctypes.c_void_p)
    for origin, w, n_groups, which_mask, message in ((0, 100, 4, 1, b"which_mask"), (0, 0, 4, 0, b"width"),
                                                     (0, 100, 0, 0, b"n_groups")):
        request = _abi.BucketRequestC(origin, w, 10, I64_MIN, I64_MAX, n_groups, which_mask)
        assert hip.lib.mdb_binned_buckets(hip.handle, ctypes.byref(seg_x), ctypes.byref(seg_y), None, ctypes.byref(request),
                                          edge_data, len(edges), data) == 1
        assert message in hip.lib.mdb_last_error()
    request = _abi.BucketRequestC(0, 100, 10, I64_MIN, I64_MAX, 4, 0)
    for arguments in ((hip.handle, ctypes.byref(seg_x), None, None, ctypes.byref(request), edge_data, len(edges), data),
                      (hip.handle, ctypes.byref(seg_x), ctypes.byref(seg_y), None, ctypes.byref(request), None, len(edges), data),
                      (hip.handle, ctypes.byref(seg_x), ctypes.byref(seg_y), None, ctypes.byref(request), edge_data, len(edges), None)):
        assert hip.lib.mdb_binned_buckets(*arguments) == 1 and b"NULL" in hip.lib.mdb_last_error()
    assert cells.tobytes() == before.tobytes()


def test_empty_input_succeeds_and_changes_nothing(hip):
    fields = cc.main_table()
    x, y = fields[0], fields[1]
    first, last = _span(fields)
    edges = bc.quantile_edges(x.values, 3)
    rng = np.random.default_rng(10)
    cells = np.frombuffer(rng.bytes(4 * 10 * 4 * CELL.itemsize), dtype=CELL).reshape(4, 10, 4).copy()
    cells["count"] = np.abs(cells["count"] >> 2) + 1
    before = cells.copy()
    empty = x.batch.slice(0, 0)
    hip.binned_buckets(empty, empty, edges, 0, 100, 10, cells=cells, n_groups=4)
    hip.binned_buckets(empty, y.batch.slice(0, 0), edges, 0, 100, 10, cells=cells, n_groups=4)
    hip.binned_buckets_list([], [], edges, 0, 100, 10, cells=cells, n_groups=4)
    # an empty range, and buckets the data does not reach
    hip.binned_buckets(x.batch, y.batch, edges, first, 1000, 10, groups=x.groups, t_lo=last + 10, t_hi=last + 1000, cells=cells)
    hip.binned_buckets_dev(x.resident(hip), y.resident(hip), edges, last + 1, 1000, 10, groups=x.groups, cells=cells)
    assert cells.tobytes() == before.tobytes()
    none = np.zeros((4, 0, 4), dtype=CELL)
    assert hip.binned_buckets(x.batch, y.batch, edges, 0, 100, 0, groups=x.groups, cells=none).shape == (4, 0, 4)
    assert hip.binned_buckets_dev(x.resident(hip), y.resident(hip), edges, 0, 100, 0, groups=x.groups, cells=none).shape == (4, 0, 4)
    assert hip.binned(empty, empty, edges, n_groups=2).tobytes() == bytes(2 * 4 * CELL.itemsize)


def _random_cases():
    """40 cases over the three tables, a fixed seed: an ordered pair of fields, a request (widths from one interval to
    the whole span, origins before, inside and after the data, ranges that cut buckets) and 1 .. 200 edges drawn from
    quantiles of x, +-0, +-inf and values outside the data."""
    rng = np.random.default_rng(20261019)
    tables = {"main": cc.main_table(), "edge": cc.edge_table(), "steps": cc.steps_table()}
    drawn = []
    for number in range(40):
        # (a cell fed by several segments needs several segments per series: the main table in most cases)
        name = "edge" if number % 13 == 3 else "steps" if number % 13 == 8 else "main"
        fields = tables[name]
        a, b = rng.choice(len(fields), 2, replace=False)
        x, y = fields[a], fields[b]
        wanted = int(rng.integers(1, 201))
        if name == "edge":   # (its series lie around 0 and around an epoch-scale timestamp: requests that reach them)
            epoch = 1658671178037
            origin, width, n_buckets, t_lo, t_hi = [(0, 100, 40, I64_MIN, I64_MAX), (-35, 250, 24, 150, 950),
                                                    (epoch - 1000, 3000, 30, I64_MIN, I64_MAX),
                                                    (epoch, 50_000, 10, epoch + 100_500, epoch + 300_400),
                                                    (0, 1 << 40, 3, I64_MIN, I64_MAX)][int(rng.integers(0, 5))]
        else:
            first, last = _span(fields)
            span = last - first + 1
            width = int(rng.choice([INTERVAL, 7 * INTERVAL, int(rng.integers(INTERVAL, span)), span], p=[0.1, 0.2, 0.4, 0.3]))
            origin = int(first + rng.choice([-width - 17, -5, 0, span // 3]))
            if number in (5, 25):   # (buckets that begin after the data)
                origin = first + span + 10
            # (at most 400 000 cells a case: narrow buckets then cover the front of the data only)
            n_buckets = int(min(max((last - origin) // width + int(rng.integers(0, 3)), 1), 400_000 // (4 * (wanted + 1))))
            t_lo, t_hi = I64_MIN, I64_MAX
            if rng.random() < 0.5:
                t_lo, t_hi = int(first + rng.integers(0, span // 10)), int(last - rng.integers(0, span // 3))
        finite = x.values[np.isfinite(x.values)]
        candidates = np.concatenate([np.quantile(finite.astype(np.float64), rng.random(wanted)).astype(np.float32),
                                     np.array([-0.0, 0.0, -np.inf, np.inf, finite.min() - 10.0, finite.max() + 10.0],
                                              dtype=np.float32)])
        chosen = candidates[rng.permutation(len(candidates))[:wanted]]
        keys, index = np.unique(bc.keys_of(chosen), return_index=True)   # (distinct and ascending in totalOrder)
        edges = chosen[index]
        grouped = bool(rng.random() < 0.5)
        drawn.append((name, int(a), int(b), edges, origin, width, n_buckets, t_lo, t_hi, grouped))
    return tables, drawn


def test_randomised_requests_against_the_oracle(hip):
    tables, drawn = _random_cases()
    expectations = []
    for name, a, b, edges, origin, width, n_buckets, t_lo, t_hi, grouped in drawn:
        x, y = tables[name][a], tables[name][b]
        groups, n_groups = (x.groups, len(x.parts)) if grouped else (None, 1)
        expectations.append(bc.oracle(x, y, edges, groups, n_groups, origin, width, n_buckets, t_lo, t_hi))
    # from the oracle alone: the draw has not degenerated
    assert sum(1 for expected in expectations if (expected["segments"] > 1).any()) >= 30
    assert {len(case[3]) for case in drawn} != {1} and max(len(case[3]) for case in drawn) > 100
    for number, (case, expected) in enumerate(zip(drawn, expectations)):
        name, a, b, edges, origin, width, n_buckets, t_lo, t_hi, grouped = case
        x, y = tables[name][a], tables[name][b]
        groups, n_groups = (x.groups, len(x.parts)) if grouped else (None, 1)
        got = hip.binned_buckets(x.batch, y.batch, edges, origin, width, n_buckets, groups=groups, t_lo=t_lo, t_hi=t_hi,
                                 n_groups=n_groups)
        bc.assert_cells(got, expected, f"case {number} {name} x{a} y{b} {len(edges)} edges width {width}")
        if number % 8 == 0:
            on_device = hip.binned_buckets_dev(x.resident(hip), y.resident(hip), edges, origin, width, n_buckets,
                                               groups=groups, t_lo=t_lo, t_hi=t_hi, n_groups=n_groups)
            assert on_device.tobytes() == got.tobytes()


@pytest.mark.parametrize("eb_name", ["lossless", "rel5", "abs5"])
def test_unsorted_timestamps_take_the_points_the_other_operators_take(hip, eb_name):
    """(a consistency check) Segments whose irregular timestamps are not sorted (a malformed stream that still decodes:
    the batches of tests/test_gpu_hist_buckets.py) under MacaqueV values, residual tails and plain models, the field
    paired with itself: count equals hist_buckets' cells exactly, and the cells merged over c give the moments
    comoments_buckets has for the same pairs."""
    import cases
    from test_gpu_hist_buckets import _unsorted
    _, _, sorted_batch = cases.mixed_batch(cases.error_bounds()[eb_name], True, seed=1700 + len(eb_name), length=3_000)
    batch, changed, _ = _unsorted(sorted_batch, np.random.default_rng(17))
    assert len(changed) >= 5
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    edges = np.array([120.0, 150.0, 180.0], dtype=np.float32)
    for origin, width in ((first, (last - first) // 64 | 1), (first - 77, (last - first) // 23)):
        args = (origin, width, (last - origin) // width + 1)
        cells = hip.binned_buckets(batch, batch, edges, *args, groups=groups, n_groups=3)
        counts = hip.hist_buckets(batch, edges, *args, groups, n_groups=3)
        assert int(counts.sum()) > 2_000
        np.testing.assert_array_equal(cells["count"], counts.astype(np.int64))
        pairs = mdb.comoments_moments(hip.comoments_buckets(batch, batch, *args, groups=groups, n_groups=3), "y")
        folded = _fold_over_cells(cells)
        np.testing.assert_array_equal(folded["count"], pairs["count"])
        hit = pairs["count"] > 0
        assert (np.abs(folded["mean"][hit] - pairs["mean"][hit]) <= bc.MEAN_TOLERANCE * np.abs(pairs["mean"][hit])).all()   # (|mean| <= the largest |v|)
        assert (np.abs(folded["m2"][hit] - pairs["m2"][hit]) <= bc.M2_TOLERANCE * pairs["m2"][hit]).all()
        # x paired with itself: the mean of a cell lies within its edges
        lower = np.concatenate([[-np.inf], edges.astype(np.float64)])
        upper = np.concatenate([edges.astype(np.float64), [np.inf]])
        filled = cells["count"] > 0
        assert (cells["mean"] >= lower)[filled].all() and (cells["mean"] <= upper)[filled].all()
