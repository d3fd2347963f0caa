"""Rolling windows over per-bucket cells on the device (mdb_roll_cells_dev): the same bytes as the host form
(mdb_roll_cells) for all eight kinds over the shape grid of tests/test_roll_cpu.py and the shapes that take other
paths (several waves of blocks per column, several waves of inner lanes, no suffix pass, a single block), an exact
capacity with guards around `out`; and end to end on segments: every *_buckets_dev operator at width w rolled with
window 6 against the same operator called directly at width 6 w, one bucket per window - byte-identical where the
operator's cells are integers or selections, within the case modules' tolerances against their oracles elsewhere.

Two forms are compared by roll_cases.image: every bit of every cell, except that a NaN member is compared as "a NaN"
(the merge rules leave a NaN's sign and payload to the instruction that adds or multiplies, and x86 and gfx950 make
different ones of inf - inf)."""

import numpy as np
import pytest
import torch

import binned_cases as bc
import cases
import change_cases as chc
import comoments_cases as cc
import derived_cases as dc
import dwell_cases as dwc
import integral_cases as ic
import moments_cases as mc
import modelardb_rs_amd as mdb
import roll_cases as rc
import trend_cases as tc

pytestmark = pytest.mark.gpu

KIND_NAMES = list(rc.KINDS)
GUARD = 256   # bytes on either side of `out`
SUM_TOLERANCE = 1e-5   # tests/test_gpu_agg_buckets.py's, of the sum of magnitudes (the values here are positive)


def roll_dev(context, kind, cells, window, stride):
    """mdb_roll_cells_dev on `cells` [n_outer][n_buckets][n_inner] with a capacity of exactly the cells needed; the
    guard regions around `out` must come back untouched."""
    cells = np.ascontiguousarray(cells)
    n_outer, n_buckets, n_inner = cells.shape
    n_windows = rc.n_windows_of(n_buckets, window, stride)
    n_out, size = n_outer * n_windows * n_inner, cells.dtype.itemsize
    dev_cells = context.upload_array(cells)
    dev_out = context.upload_array(np.full(2 * GUARD + n_out * size, 0xC3, dtype=np.uint8))
    try:
        assert context.roll_cells_dev(rc.KINDS[kind], dev_cells, n_outer, n_buckets, n_inner, window, stride,
                                      dev_out + GUARD, n_out) == n_windows
        raw = context.download_array(dev_out, 2 * GUARD + n_out * size, np.uint8)
        assert (raw[:GUARD] == 0xC3).all() and (raw[GUARD + n_out * size:] == 0xC3).all(), "a guard was written"
        assert context.download_array(dev_cells, cells.size, cells.dtype).tobytes() == cells.tobytes()
    finally:
        context.dev_free(dev_cells)
        context.dev_free(dev_out)
    return raw[GUARD:GUARD + n_out * size].view(cells.dtype).reshape(n_outer, n_windows, n_inner)


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_device_form_equals_the_host_form_on_the_cpu_grid(hip, kind):
    big = rc.big(kind)
    for window, stride, n_buckets in rc.shape_grid():
        for n_outer, n_inner in ((1, 1), (1, 3), (5, 1), (5, 3)):
            cells = np.ascontiguousarray(big[:n_outer, :n_buckets, :n_inner])
            got = roll_dev(hip, kind, cells, window, stride)
            assert rc.image(kind, got) == rc.image(kind, mdb.roll_cells(cells, window, stride)), \
                (kind, window, stride, n_buckets, n_outer, n_inner)


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_shapes_that_take_other_paths(hip, kind):
    """4097 buckets at window 64: 65 blocks a column, more than a wave of them, the last of one bucket; stride 64 and
    128: no suffix pass; window = n_buckets: one block; window 1: a strided copy."""
    cells = rc.random_cells(kind, (2, 4097, 2), seed=2080)
    hip.profile_enable(True)
    for window, stride, suffix in ((64, 1, True), (64, 5, True), (64, 64, False), (64, 128, False), (4097, 1, False),
                                   (1, 3, False), (4096, 1, True)):
        hip.profile_reset()
        got = roll_dev(hip, kind, cells, window, stride)
        kernels = hip.profile()
        assert "k_roll_windows" in kernels and kernels["k_roll_windows"][0] == 1, sorted(kernels)
        assert ("k_roll_suffix" in kernels) == suffix, (window, stride, sorted(kernels))
        assert rc.image(kind, got) == rc.image(kind, mdb.roll_cells(cells, window, stride)), (kind, window, stride)
    hip.profile_enable(False)
    strided = roll_dev(hip, kind, cells, 1, 3)
    assert strided.tobytes() == np.ascontiguousarray(cells[:, ::3]).tobytes()


def test_more_than_two_waves_of_inner_lanes(hip):
    cells = rc.random_cells("u64", (3, 150, 130), seed=2081)
    for window, stride in ((7, 1), (7, 7), (64, 3), (150, 1)):
        got = roll_dev(hip, "u64", cells, window, stride)
        assert got.tobytes() == mdb.roll_cells(cells, window, stride).tobytes(), (window, stride)


def test_two_runs_a_clone_and_a_callers_stream_give_the_same_bytes(hip):
    for kind in ("moments", "change", "m4"):
        cells = rc.random_cells(kind, (3, 1000, 2), seed=2082)
        first = roll_dev(hip, kind, cells, 60, 1)
        assert roll_dev(hip, kind, cells, 60, 1).tobytes() == first.tobytes()
        clone = hip.clone()
        stream = torch.cuda.Stream()
        try:
            assert roll_dev(clone, kind, cells, 60, 1).tobytes() == first.tobytes()
            clone.set_stream(stream.cuda_stream)
            assert roll_dev(clone, kind, cells, 60, 1).tobytes() == first.tobytes()
        finally:
            clone.close()
            del stream


def test_scratch_refused_under_a_limit_names_the_bytes(hip):
    cells = rc.random_cells("change", (4, 1000, 1), seed=2083)
    clone = hip.clone()
    try:
        clone.set_scratch_limit(1 << 16)
        needed = 4 * 960 * 64   # the blocks but the last of every column: 16 blocks of 60 buckets, 64 B a cell
        with pytest.raises(mdb.HipError, match=str(needed)):
            roll_dev(clone, "change", cells, 60, 1)
        got = roll_dev(clone, "change", cells, 60, 60)   # (no suffix folds: nothing to refuse)
        assert rc.image("change", got) == rc.image("change", mdb.roll_cells(cells, 60, 60))
        clone.set_scratch_limit(0)
        assert rc.image("change", roll_dev(clone, "change", cells, 60, 1)) == rc.image("change", mdb.roll_cells(cells, 60, 1))
    finally:
        clone.close()


# ---- end to end on segments ---------------------------------------------------------------------------------------

WINDOW = 6
_TABLE = {}


def _table():
    """Two fields of three series - regular, irregular, regular timestamps - whose levels and slopes change every 5 to
    40 points, each series a group: under 1 % relative some 200 segments of PMC-Mean and Swing with residual tails,
    lossless some 70 of Swing and MacaqueV. The tests roll the first field at stride 1 and the second at stride 4."""
    if not _TABLE:
        series = [cc._series(4000, False, (41, 42), segment_length_range=(5, 41)),
                  cc._series(3200, True, (51, 52), segment_length_range=(5, 41), t0=20_000),
                  cc._series(2800, False, (61, 62), segment_length_range=(5, 41), t0=60_000)]
        bounds = cases.error_bounds()
        _TABLE["fields"] = cc.table(series, [bounds["rel1"], bounds["lossless"]])
        assert len(_TABLE["fields"][0].batch) >= 200 and len(set(_TABLE["fields"][1].batch.model_type_id.tolist())) >= 2
    return _TABLE["fields"]


def _fields(stride):
    """(the field the operators of one field run on, its partner) with their resident batches' order."""
    x, y = _table()
    return (x, y, 0) if stride == 1 else (y, x, 1)


def _grid_of(field):
    first, last = int(field.ts.min()), int(field.ts.max())
    width = 37 * cc.INTERVAL + 11   # (no multiple of the sampling interval)
    origin = first - 5 * width - 3
    return origin, width, (last - origin) // width + 3


def _phases(stride):
    """(phase p, the windows k with k * stride % WINDOW == p)."""
    return sorted({(k * stride) % WINDOW for k in range(WINDOW)})


def _compare(n_buckets, stride, rolled, direct_at, check):
    """rolled: [groups][n_windows][...]. For every phase p the windows that start at p + WINDOW * q are the buckets q of
    the direct call at origin + p * w and width WINDOW * w: check(rolled windows, phase, n_direct_buckets)."""
    n_windows = rc.n_windows_of(n_buckets, WINDOW, stride)
    assert rolled.shape[1] == n_windows
    seen = 0
    for phase in _phases(stride):
        starts = np.arange(phase, n_buckets - WINDOW + 1, WINDOW)
        starts = starts[starts % stride == 0]
        if len(starts) == 0:
            continue
        n_direct = int(starts[-1] - phase) // WINDOW + 1
        direct = direct_at(phase, n_direct)
        picked = (starts - phase) // WINDOW
        check(rolled[:, starts // stride], direct, picked, f"stride {stride} phase {phase}")
        seen += len(starts)
    assert seen == n_windows


def _picked(expected, picked):
    """An oracle's cells (arrays [groups][buckets][...] by member, beside plain figures) at the buckets `picked`."""
    return {key: value[:, picked] if isinstance(value, np.ndarray) else value for key, value in expected.items()}


@pytest.fixture(scope="module")
def resident(hip):
    x, y = _table()
    yield x.resident(hip), y.resident(hip)
    x.free()
    y.free()


def _rolled(hip, kind, cells, stride):
    shape = cells.shape
    flat = cells.reshape(shape[0], shape[1], -1)
    got = roll_dev(hip, kind, flat, WINDOW, stride)
    return got.reshape((shape[0], got.shape[1]) + shape[2:])


@pytest.mark.parametrize("stride", [1, 4])
def test_integer_and_selection_operators_roll_to_the_direct_calls_bytes(hip, resident, stride):
    x, _, first = _fields(stride)
    dev_x = resident[first]
    origin, width, n_buckets = _grid_of(x)
    edges = dwc.edges_through(x.values, 5)
    operators = {
        "m4": ("m4", lambda o, w, n: hip.m4_buckets_dev(dev_x, o, w, n, groups=x.groups, n_groups=3)),
        "hist": ("u64", lambda o, w, n: hip.hist_buckets_dev(dev_x, edges, o, w, n, groups=x.groups, n_groups=3)),
        "dwell": ("u64", lambda o, w, n: hip.dwell_buckets_dev(dev_x, edges, o, w, n, groups=x.groups, n_groups=3)),
        "transit": ("u64", lambda o, w, n: hip.transit_buckets_dev(dev_x, edges, o, w, n, groups=x.groups, n_groups=3)),
    }
    for name, (kind, call) in operators.items():
        fine = call(origin, width, n_buckets)
        assert fine.shape[:2] == (3, n_buckets) and (fine.view(np.uint8) != 0).any(), name

        def check(windows, direct, picked, context):
            assert np.ascontiguousarray(windows).tobytes() == np.ascontiguousarray(direct[:, picked]).tobytes(), (name, context)

        _compare(n_buckets, stride, _rolled(hip, kind, fine, stride),
                 lambda phase, n: call(origin + phase * width, WINDOW * width, n), check)


@pytest.mark.parametrize("stride", [1, 4])
def test_exact_members_of_change_integral_and_agg_roll_to_the_direct_calls(hip, resident, stride):
    x, _, first = _fields(stride)
    dev_x = resident[first]
    origin, width, n_buckets = _grid_of(x)
    operators = {
        "change": ("change", lambda o, w, n: hip.change_buckets_dev(dev_x, o, w, n, groups=x.groups, n_groups=3),
                   ("count", "n_fall", "duration", "max_rise", "max_fall"), ("rise", "fall", "reset_sum")),
        "integral": ("integral", lambda o, w, n: hip.integral_buckets_dev(dev_x, o, w, n, groups=x.groups, n_groups=3),
                     ("duration",), ("integral",)),
        "agg": ("agg", lambda o, w, n: hip.agg_buckets_dev(dev_x, o, w, n, groups=x.groups, n_groups=3),
                ("count", "min", "max"), ("sum",)),
    }
    for name, (kind, call, exact, sums) in operators.items():
        fine = call(origin, width, n_buckets)

        def check(windows, direct, picked, context):
            for member in exact:   # (min and max with ==: the sign of a zero follows the order of the buckets)
                np.testing.assert_array_equal(windows[member], direct[member][:, picked], err_msg=f"{name} {member} {context}")
            for member in sums:    # (positive terms only: the direct sum is the sum of magnitudes)
                error = np.abs(windows[member] - direct[member][:, picked])
                assert (error <= SUM_TOLERANCE * np.abs(direct[member][:, picked])).all(), (name, member, context)

        _compare(n_buckets, stride, _rolled(hip, kind, fine, stride),
                 lambda phase, n: call(origin + phase * width, WINDOW * width, n), check)
    # and the float sums against the modules' oracles, by their own assert_cells
    fine = hip.change_buckets_dev(dev_x, origin, width, n_buckets, groups=x.groups, n_groups=3)
    _compare(n_buckets, stride, _rolled(hip, "change", fine, stride),
             lambda phase, n: chc.oracle(x, x.groups, 3, origin + phase * width, WINDOW * width, n),
             lambda windows, expected, picked, context: chc.assert_cells(
                 np.ascontiguousarray(windows), _picked(expected, picked), f"change {context}"))
    fine = hip.integral_buckets_dev(dev_x, origin, width, n_buckets, groups=x.groups, n_groups=3)
    _compare(n_buckets, stride, _rolled(hip, "integral", fine, stride),
             lambda phase, n: ic.oracle(x, x.groups, 3, origin + phase * width, WINDOW * width, n, ic.LINEAR),
             lambda windows, expected, picked, context: ic.assert_cells(
                 np.ascontiguousarray(windows), _picked(expected, picked), f"integral {context}"))


@pytest.mark.parametrize("stride", [1, 4])
def test_float_operators_roll_within_their_modules_tolerances(hip, resident, stride):
    x, y, first = _fields(stride)
    dev_x, dev_y = resident[first], resident[1 - first]
    origin, width, n_buckets = _grid_of(x)
    edges = dwc.edges_through(x.values, 3)
    batch = x.batch
    operators = {
        "moments": ("moments", lambda: hip.moments_buckets_dev(dev_x, origin, width, n_buckets, groups=x.groups, n_groups=3),
                    lambda o, w, n: mc.oracle(batch, x.groups, 3, o, w, n), mc.assert_cells),
        "comoments": ("comoments", lambda: hip.comoments_buckets_dev(dev_x, dev_y, origin, width, n_buckets, groups=x.groups, n_groups=3),
                      lambda o, w, n: cc.oracle(x, y, x.groups, 3, o, w, n), cc.assert_cells),
        "trend": ("comoments", lambda: hip.trend_buckets_dev(dev_x, origin, width, n_buckets, groups=x.groups, n_groups=3),
                  lambda o, w, n: tc.oracle(x, x.groups, 3, o, w, n), cc.assert_cells),
        "derived": ("derived", lambda: hip.derived_buckets_dev(dev_x, dev_y, dc.expression("product"), origin, width, n_buckets,
                                                               groups=x.groups, n_groups=3),
                    lambda o, w, n: dc.oracle(x, y, "product", x.groups, 3, o, w, n), dc.assert_cells),
        "binned": ("moments", lambda: hip.binned_buckets_dev(dev_x, dev_y, edges, origin, width, n_buckets, groups=x.groups, n_groups=3),
                   lambda o, w, n: bc.oracle(x, y, edges, x.groups, 3, o, w, n), bc.assert_cells),
    }
    for name, (kind, call, oracle, assert_cells) in operators.items():
        fine = call()
        assert fine.shape[:2] == (3, n_buckets), name
        if name == "trend":
            # A trend cell's x is the offset inside ITS bucket (mdb.h): before cells of different buckets meet, mean_x is
            # moved to one origin - bucket b's by b * width, exact in integers below 2^53 - and a window's back to its
            # own first instant afterwards. m2_x and c_xy do not depend on the shift.
            fine["mean_x"] += np.where(fine["count"] > 0, np.arange(n_buckets).reshape(1, -1) * float(width), 0.0)
        rolled = _rolled(hip, kind, fine, stride)
        if name == "trend":
            rolled["mean_x"] -= np.where(rolled["count"] > 0, np.arange(rolled.shape[1]).reshape(1, -1) * float(stride * width), 0.0)
        _compare(n_buckets, stride, rolled,
                 lambda phase, n: oracle(origin + phase * width, WINDOW * width, n),
                 lambda windows, expected, picked, context: assert_cells(
                     np.ascontiguousarray(windows), _picked(expected, picked), f"{name} {context}"))
