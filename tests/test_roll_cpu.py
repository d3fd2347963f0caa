"""CPU-side checks of the rolling windows (mdb_roll_windows, mdb_roll_cells, mdb_roll_cells_dev up to the device): the
entry points in the built library, the header, the ctypes mirror and the Rust binding; the layout of mdb_roll_request
and the MDB_ROLL_* constants everywhere; mdb_roll_cells against the Python restatement of the rule (tests/roll_cases.py)
bit for bit for every kind over a grid of shapes; the windows that start a block against the chained *_merge_n left
fold; uint64 against numpy's sliding sum; M4 and the aggregates' count / min / max against a brute-force recomputation
from point sets; moments, comoments and derived cells against exact references within their modules' tolerances; every
error; and the host side (modelardb-rs_amd/csrc/mdb_roll_host.cpp) driven by a stand-alone program, plain and under
AddressSanitizer + UBSan (tests/roll_host).

"Bit for bit" is roll_cases.image: every bit of every cell, with one thing left open as the merge rules leave it open -
WHICH NaN a float member holds when it is one. The generators put infinities and NaNs into means and sums, and of
inf - inf, or of two NaN operands, the compiler's operand order and the instruction set decide sign and payload: the
same merge function inlined into mdb_roll_host.cpp and into mdb_moments_host.cpp already differs there. That the member
is a NaN is compared; M4 cells (selections) and uint64 counters are compared as raw bytes."""

import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import comoments_cases as cc
import derived_cases as dc
import moments_cases as mc
import modelardb_rs_amd as mdb
import roll_cases as rc
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "roll_host")
NAMES = ("mdb_roll_windows", "mdb_roll_cells", "mdb_roll_cells_dev")
OFFSETS = {"kind": 0, "flags": 4, "n_outer": 8, "n_buckets": 16, "n_inner": 24, "window": 32, "stride": 40}
KIND_NAMES = list(rc.KINDS)
BIG, shape_grid, _big = rc.BIG, rc.shape_grid, rc.big


def test_entry_points_exported_declared_and_bound():
    library = _abi.HIP_LIBRARY_PATH
    assert os.path.exists(library), "build() first"
    exported = subprocess.run(["nm", "-D", "--defined-only", library], check=True, capture_output=True,
                              text=True).stdout.split()
    header = open(os.path.join(REPO_ROOT, "include", "mdb.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    binding = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in exported, name
        assert re.search(rf"\bint {name}\(", header), name
        assert re.search(rf"pub fn {name}\(", rust), name
        assert name in _abi.hip_symbol_names(), name
        assert name.endswith("_dev") or f"sys::{name}(" in binding, name
    declared = set(re.findall(r"\b(mdb_\w+)\(", header))
    bound = set(re.findall(r"pub fn (mdb_\w+)\(", rust))
    listed = {name for name in exported if name.startswith("mdb_")}
    assert {name for name in declared | bound | listed if "roll" in name} == set(NAMES)
    assert declared == bound, declared ^ bound
    for name in NAMES:   # (other operators' CPU tests partition the symbol table by these substrings)
        assert not any(word in name for word in ("derived", "comoments", "binned", "trend", "change", "dwell", "transit",
                                                 "episodes", "integral", "moments", "m4", "hist", "sample", "agg"))


def test_layouts_and_constants_agree_everywhere():
    text = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    mirror = _abi.RollRequestC
    assert ctypes.sizeof(mirror) == 48
    assert [name for name, _ in mirror._fields_] == list(OFFSETS)
    assert re.search(r"MDB_LAYOUT_ASSERT\(sizeof\(mdb_roll_request\) == 48\)", text)
    assert re.search(r"size_of::<mdb_roll_request>\(\) == 48\b", rust)
    for name, offset in OFFSETS.items():
        assert getattr(mirror, name).offset == offset, name
        assert re.search(rf"MDB_LAYOUT_ASSERT\(offsetof\(mdb_roll_request, {name}\) == {offset}\)", text), name
        assert re.search(rf"offset_of!\(mdb_roll_request, {name}\) == {offset}\b", rust), name
    rust_request = re.search(r"pub struct mdb_roll_request \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", rust_request) == [("kind", "u32"), ("flags", "u32")] + [
        (name, "u64") for name in list(OFFSETS)[2:]]
    assert sorted(rc.KINDS.values()) == list(range(8)) and set(mdb.ROLL_KINDS) == set(rc.KINDS.values())
    for name, value in rc.KINDS.items():
        assert re.search(rf"#define MDB_ROLL_{name.upper()}\s+{value}u", text), name
        assert re.search(rf"pub const MDB_ROLL_{name.upper()}: u32 = {value};", rust), name
        assert getattr(mdb, f"MDB_ROLL_{name.upper()}") == value == getattr(_abi, f"MDB_ROLL_{name.upper()}")
        assert mdb.ROLL_KINDS[value].itemsize == rc.CELL_SIZES[name]
        assert mdb.roll_kind_of(mdb.ROLL_KINDS[value]) == value
    with pytest.raises(ValueError):
        mdb.roll_kind_of(mdb.SAMPLE_CELL_DTYPE)   # (instants are not intervals: mdb_format.h says so)
    assert "mdb_sample_cell has no kind" in text


def test_window_counts():
    for n_buckets, window, stride in ((0, 1, 1), (5, 6, 1), (6, 6, 1), (7, 6, 1), (7, 6, 2), (8, 6, 2), (200, 7, 8),
                                      (1 << 40, 60, 1), ((1 << 61) - 1, 1, 1), ((1 << 61) - 1, (1 << 61) - 1, 5)):
        assert mdb.roll_windows(n_buckets, window, stride) == rc.n_windows_of(n_buckets, window, stride)
    with pytest.raises(mdb.HipError, match="overflows"):   # (counted in 8-byte cells: 2^61 of them are 2^64 bytes)
        mdb.roll_windows(1 << 61, 1, 1)
    for window, stride in ((0, 1), (1, 0)):
        with pytest.raises(mdb.HipError):
            mdb.roll_windows(10, window, stride)


@functools.lru_cache(maxsize=None)
def _folds(kind, window, n_buckets):
    return rc.folds(kind, np.ascontiguousarray(_big(kind)[:, :n_buckets]), window)


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_host_form_equals_the_restated_rule_bit_for_bit(kind):
    compared = 0
    for window, stride, n_buckets in shape_grid():
        prefix, suffix = _folds(kind, window, n_buckets)
        expected = rc.windows_from(kind, prefix, suffix, window, stride)
        for n_outer in (1, 5):
            for n_inner in (1, 3):
                cells = np.ascontiguousarray(_big(kind)[:n_outer, :n_buckets, :n_inner])
                before = cells.tobytes()
                got = mdb.roll_cells(cells, window, stride)
                want = np.ascontiguousarray(expected[:n_outer, :, :n_inner])
                assert got.shape == want.shape == (n_outer, rc.n_windows_of(n_buckets, window, stride), n_inner)
                assert rc.image(kind, got) == rc.image(kind, want), (kind, window, stride, n_buckets, n_outer, n_inner)
                assert cells.tobytes() == before
                compared += got.size
    assert compared > 10_000
    # a 1-D array is one column; an explicit kind is the same call
    column = np.ascontiguousarray(_big(kind)[2, :50, 1])
    assert rc.image(kind, mdb.roll_cells(column, 7, 3)) == rc.image(kind, rc.reference(kind, column.reshape(1, 50, 1), 7, 3))
    assert mdb.roll_cells(column, 7, 3, kind=rc.KINDS[kind]).tobytes() == mdb.roll_cells(column, 7, 3).tobytes()
    # trailing axes are one inner axis
    square = np.ascontiguousarray(_big(kind)[:, :36, :]).reshape(5, 9, 2, 2, 3)
    assert rc.image(kind, mdb.roll_cells(square, 4, 2)) == rc.image(kind, rc.reference(kind, square.reshape(5, 9, 12), 4, 2))
    assert mdb.roll_cells(square, 4, 2).shape == (5, 3, 2, 2, 3)


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_windows_that_start_a_block_are_the_chained_left_fold(kind):
    cells = _big(kind)
    for window, stride in ((1, 1), (2, 1), (3, 2), (7, 1), (7, 7), (7, 14), (64, 1), (65, 5), (200, 1)):
        got = mdb.roll_cells(cells, window, stride)
        checked = 0
        for k in range(got.shape[1]):
            if (k * stride) % window == 0:
                assert rc.image(kind, got[:, k]) == rc.image(kind, rc.left_fold(kind, cells, k * stride, window)), (window, stride, k)
                checked += 1
        assert checked >= 1


def test_u64_is_numpys_sliding_sum_with_wrap_around():
    cells = _big("u64")
    assert (cells > (1 << 63)).any()
    for window, stride in ((1, 1), (2, 1), (3, 2), (7, 1), (64, 3), (65, 1), (200, 1)):
        with np.errstate(over="ignore"):
            total = np.concatenate([np.zeros((5, 1, 3), dtype=np.uint64), np.cumsum(cells, axis=1, dtype=np.uint64)], axis=1)
            starts = np.arange(rc.n_windows_of(200, window, stride)) * stride
            expected = total[:, starts + window] - total[:, starts]
        np.testing.assert_array_equal(mdb.roll_cells(cells, window, stride), expected)


def _point_sets(rng, n_buckets, most=12):
    """Per bucket a set of points (timestamps inside the bucket, values with ties, +-0 and NaNs); some buckets empty."""
    sets = []
    for b in range(n_buckets):
        n = 0 if rng.random() < 0.2 else int(rng.integers(1, most))
        timestamps = 1000 * b + rng.integers(0, 1000, n)
        values = rng.choice(np.array([-2.5, -0.0, 0.0, 1.0, 1.0, 7.25, np.nan, 3.0e38], dtype=np.float32), n)
        sets.append((timestamps.astype(np.int64), values.astype(np.float32)))
    return sets


def test_m4_windows_are_those_of_the_windows_points_exactly():
    rng = np.random.default_rng(2071)
    n_buckets = 90
    sets = _point_sets(rng, n_buckets)
    cells = np.array([rc.m4_cell_of(*points) for points in sets], dtype=mdb.M4_CELL_DTYPE).reshape(1, n_buckets, 1)
    for window, stride in ((1, 1), (6, 1), (6, 4), (7, 7), (64, 1), (90, 1)):
        got = mdb.roll_cells(cells, window, stride)
        for k in range(got.shape[1]):
            inside = sets[k * stride:k * stride + window]
            expected = rc.m4_cell_of(np.concatenate([t for t, _ in inside]), np.concatenate([v for _, v in inside]))
            assert got[0, k, 0].tobytes() == expected.tobytes(), (window, stride, k)


def test_agg_count_min_max_are_those_of_the_windows_points_exactly():
    rng = np.random.default_rng(2072)
    n_buckets = 90
    sets = _point_sets(rng, n_buckets)
    cells = mdb.fresh_agg_states((1, n_buckets, 1))

    def state_of(values):
        numbers = values[~np.isnan(values)]
        low = min(rc.FLT_MAX, numbers.min()) if len(numbers) else rc.FLT_MAX
        high = max(-rc.FLT_MAX, numbers.max()) if len(numbers) else -rc.FLT_MAX
        return len(values), np.float32(low), np.float32(high)

    for b, (_, values) in enumerate(sets):
        count, low, high = state_of(values)
        cells[0, b, 0] = (math.fsum(values[~np.isnan(values)].astype(np.float64)), count, low, high)
    for window, stride in ((1, 1), (6, 1), (6, 4), (7, 7), (64, 1), (90, 1)):
        got = mdb.roll_cells(cells, window, stride)
        for k in range(got.shape[1]):
            count, low, high = state_of(np.concatenate([v for _, v in sets[k * stride:k * stride + window]]))
            assert (got["count"][0, k, 0], got["min"][0, k, 0], got["max"][0, k, 0]) == (count, low, high), (window, stride, k)


def _runs(rng, values, n_buckets):
    """`values` cut into n_buckets runs in order, a few of them empty."""
    cuts = np.sort(rng.integers(0, len(values) + 1, n_buckets - 1))
    cuts[rng.random(n_buckets - 1) < 0.15] = cuts[0]
    cuts = np.concatenate([[0], np.sort(cuts), [len(values)]])
    return [(int(cuts[b]), int(cuts[b + 1])) for b in range(n_buckets)]


WINDOWS = ((1, 1), (2, 1), (7, 3), (64, 1), (65, 2), (120, 1))


def test_moments_windows_meet_the_modules_tolerances():
    rng = np.random.default_rng(2073)
    n_buckets = 120
    for name, (values, _) in dc.data_sets(rng, 6000).items():
        runs = _runs(rng, values, n_buckets)
        cells = mdb.fresh_moments_cells((1, n_buckets, 1))
        for b, (lo, hi) in enumerate(runs):
            if hi > lo:
                cells[0, b, 0] = (hi - lo,) + mc.cell_reference(values[lo:hi])
        for window, stride in WINDOWS:
            got = mdb.roll_cells(cells, window, stride)
            n_windows = got.shape[1]
            point_windows = np.concatenate([np.full(runs[k * stride + window - 1][1] - runs[k * stride][0], k)
                                            for k in range(n_windows)]).astype(np.int64)
            points = np.concatenate([values[runs[k * stride][0]:runs[k * stride + window - 1][1]] for k in range(n_windows)])
            expected = {key: array.reshape(1, n_windows, 1) for key, array in mc.reduce(points, point_windows, n_windows).items()}
            mc.assert_cells(got, expected, f"moments {name} window {window} stride {stride}")


def test_derived_windows_meet_the_modules_tolerances():
    rng = np.random.default_rng(2074)
    n_buckets = 120
    for name, (values, _) in dc.data_sets(rng, 6000).items():
        runs = _runs(rng, values, n_buckets)
        cells = dc.cells_of([values[lo:hi] for lo, hi in runs]).reshape(1, n_buckets, 1)
        for window, stride in WINDOWS:
            got = mdb.roll_cells(cells, window, stride)
            n_windows = got.shape[1]
            expected = {key: np.zeros((1, n_windows, 1), dtype=dtype) for key, dtype in
                        (("count", np.int64), ("mean", float), ("m2", float), ("min", np.float32), ("max", np.float32),
                         ("largest", float))}
            expected["finite"] = np.ones((1, n_windows, 1), dtype=bool)
            for k in range(n_windows):
                run = values[runs[k * stride][0]:runs[k * stride + window - 1][1]]
                expected["count"][0, k, 0] = len(run)
                if len(run):
                    mean, m2, low, high = dc.cell_reference(run)
                    expected["mean"][0, k, 0], expected["m2"][0, k, 0] = mean, m2
                    expected["min"][0, k, 0], expected["max"][0, k, 0] = low, high
                    expected["largest"][0, k, 0] = float(np.abs(run.astype(np.float64)).max())
            dc.assert_cells(got, expected, f"derived {name} window {window} stride {stride}")


def test_comoments_windows_meet_the_modules_tolerances():
    rng = np.random.default_rng(2075)
    n_buckets = 120
    for name, (x, y) in dc.data_sets(rng, 6000).items():
        runs = _runs(rng, x, n_buckets)
        cells = mdb.fresh_comoments_cells((1, n_buckets, 1))
        for b, (lo, hi) in enumerate(runs):
            if hi > lo:
                cells[0, b, 0] = (hi - lo,) + cc.cell_reference(x[lo:hi], y[lo:hi])
        for window, stride in WINDOWS:
            got = mdb.roll_cells(cells, window, stride)
            n_windows = got.shape[1]
            expected = {key: np.zeros((1, n_windows, 1)) for key in cc.MEMBERS + ("largest_x", "largest_y")}
            expected["count"] = np.zeros((1, n_windows, 1), dtype=np.int64)
            expected["finite_x"] = expected["finite_y"] = np.ones((1, n_windows, 1), dtype=bool)
            for k in range(n_windows):
                lo, hi = runs[k * stride][0], runs[k * stride + window - 1][1]
                expected["count"][0, k, 0] = hi - lo
                if hi > lo:
                    for member, value in zip(cc.MEMBERS, cc.cell_reference(x[lo:hi], y[lo:hi])):
                        expected[member][0, k, 0] = value
                    expected["largest_x"][0, k, 0] = float(np.abs(x[lo:hi].astype(np.float64)).max())
                    expected["largest_y"][0, k, 0] = float(np.abs(y[lo:hi].astype(np.float64)).max())
            cc.assert_cells(got, expected, f"comoments {name} window {window} stride {stride}")


def test_windows_of_equal_values_keep_a_zero_m2_and_their_mean_exactly():
    value = float(np.float32(1234.567))
    rng = np.random.default_rng(2076)
    counts = rng.integers(0, 50, (2, 150, 1))
    moments = mdb.fresh_moments_cells(counts.shape)
    moments["count"], moments["mean"] = counts, np.where(counts > 0, value, 0.0)
    derived = mdb.fresh_derived_cells(counts.shape)
    derived["count"], derived["mean"] = counts, np.where(counts > 0, value, 0.0)
    derived["min"] = derived["max"] = np.where(counts > 0, np.float32(value), np.float32(0.0))
    comoments = mdb.fresh_comoments_cells(counts.shape)
    comoments["count"] = counts
    comoments["mean_x"], comoments["mean_y"] = np.where(counts > 0, value, 0.0), np.where(counts > 0, -value, 0.0)
    for window, stride in WINDOWS:
        totals = mdb.roll_cells(counts.astype(np.uint64), window, stride).astype(np.int64)
        hit = totals > 0
        assert hit.any()
        got = mdb.roll_cells(moments, window, stride)
        np.testing.assert_array_equal(got["count"], totals)
        assert (got["m2"] == 0.0).all() and (got["mean"][hit] == value).all()
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * 24)
        got = mdb.roll_cells(derived, window, stride)
        assert (got["m2"] == 0.0).all() and (got["mean"][hit] == value).all()
        assert (got["min"][hit] == np.float32(value)).all() and (got["max"][hit] == np.float32(value)).all()
        got = mdb.roll_cells(comoments, window, stride)
        assert (got["m2_x"] == 0.0).all() and (got["m2_y"] == 0.0).all() and (got["c_xy"] == 0.0).all()
        assert (got["mean_x"][hit] == value).all() and (got["mean_y"][hit] == -value).all()


def test_a_window_over_fresh_cells_only_is_a_fresh_cell():
    for kind in KIND_NAMES:
        fresh = mdb.fresh_agg_states((2, 20, 2)) if kind == "agg" else np.zeros((2, 20, 2), dtype=rc.dtype_of(kind))
        got = mdb.roll_cells(fresh, 6, 3)
        assert got.shape == (2, 5, 2) and got.tobytes() == fresh[:, :5].tobytes(), kind


def _request(kind=mdb.MDB_ROLL_MOMENTS, flags=0, n_outer=2, n_buckets=10, n_inner=1, window=3, stride=1):
    return _abi.RollRequestC(kind, flags, n_outer, n_buckets, n_inner, window, stride)


def test_every_error_leaves_out_untouched_and_names_its_cause():
    library = mdb.load_hip_library()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced: every check comes before the device is used)
    cells = mdb.fresh_moments_cells(40)
    out = np.frombuffer(bytes([0xA5]) * (24 * 40), dtype=mdb.MOMENTS_CELL_DTYPE).copy()
    before = out.tobytes()
    inside = cells.ctypes.data + 24 * 5   # (out overlapping cells)
    wrong = [(_request(kind=8), cells.ctypes.data, out.ctypes.data, 40, b"kind"),
             (_request(flags=1), cells.ctypes.data, out.ctypes.data, 40, b"flag"),
             (_request(window=0), cells.ctypes.data, out.ctypes.data, 40, b"window"),
             (_request(stride=0), cells.ctypes.data, out.ctypes.data, 40, b"stride"),
             (_request(n_outer=1 << 40, n_buckets=1 << 30), cells.ctypes.data, out.ctypes.data, 40, b"overflows"),
             (_request(n_outer=1 << 61, n_buckets=1, n_inner=1, window=1), cells.ctypes.data, out.ctypes.data, 40, b"overflows"),
             (_request(n_outer=1 << 32, n_buckets=1 << 31, n_inner=2, window=1), cells.ctypes.data, out.ctypes.data, 40, b"overflows"),
             (_request(), cells.ctypes.data, out.ctypes.data, 15, b"16 cells"),
             (_request(), cells.ctypes.data, inside, 40, b"overlap"),
             (_request(), cells.ctypes.data, cells.ctypes.data, 40, b"overlap"),
             (_request(), cells.ctypes.data + 4, out.ctypes.data, 40, b"aligned"),
             (_request(), None, out.ctypes.data, 40, b"NULL"),
             (_request(), cells.ctypes.data, None, 40, b"NULL")]
    for request, cells_pointer, out_pointer, capacity, message in wrong:
        for call in (lambda: library.mdb_roll_cells(ctypes.byref(request), cells_pointer, out_pointer, capacity),
                     lambda: library.mdb_roll_cells_dev(fake_context, ctypes.byref(request), cells_pointer, out_pointer, capacity)):
            assert call() == 1
            assert message in library.mdb_last_error(), (message, library.mdb_last_error())
            assert out.tobytes() == before and cells.tobytes() == bytes(24 * 40)
    assert library.mdb_roll_cells(None, cells.ctypes.data, out.ctypes.data, 40) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_roll_cells_dev(fake_context, None, cells.ctypes.data, out.ctypes.data, 40) == 1
    assert b"NULL" in library.mdb_last_error()
    assert library.mdb_roll_cells_dev(None, ctypes.byref(_request()), cells.ctypes.data, out.ctypes.data, 40) == 1
    assert b"NULL" in library.mdb_last_error()
    n_windows = ctypes.c_uint64(99)
    assert library.mdb_roll_windows(None, ctypes.byref(n_windows)) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_roll_windows(ctypes.byref(_request()), None) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_roll_windows(ctypes.byref(_request(kind=9)), ctypes.byref(n_windows)) == 1 and n_windows.value == 99
    # the empty cases succeed, write nothing and need neither capacity nor the device
    for request in (_request(n_outer=0), _request(n_buckets=0), _request(n_inner=0), _request(n_buckets=2, window=3)):
        assert library.mdb_roll_cells(ctypes.byref(request), cells.ctypes.data, out.ctypes.data, 0) == 0
        assert library.mdb_roll_cells_dev(fake_context, ctypes.byref(request), cells.ctypes.data, out.ctypes.data, 0) == 0
    assert out.tobytes() == before
    # the Python form: the wrong type for a kind, no bucket axis
    with pytest.raises(ValueError):
        mdb.roll_cells(cells, 3, kind=mdb.MDB_ROLL_U64)
    with pytest.raises(ValueError):
        mdb.roll_cells(np.zeros(4, dtype=np.float32), 3)
    with pytest.raises(mdb.HipError, match="window"):
        mdb.roll_cells(cells, 0)
    assert mdb.roll_cells(cells[:2], 3).shape == (0,)
    assert mdb.roll_cells(np.zeros((0, 9, 2), dtype=np.uint64), 3).shape == (0, 7, 2)


@pytest.fixture(scope="module")
def built():
    done = subprocess.run(["make", "-C", HERE, "all"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


@pytest.mark.parametrize("flavour", ["plain", "asan"])
def test_host_side_without_a_gpu(built, flavour):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    done = subprocess.run([os.path.join(HERE, "_build", f"check_{flavour}")], capture_output=True, text=True, env=env,
                          timeout=300)
    output = done.stdout + done.stderr
    assert done.returncode == 0, output[-4000:]
    assert output.startswith("ok: ") or "\nok: " in output, output[-4000:]
    for report in ("ERROR: AddressSanitizer", "runtime error:", "MISMATCH"):
        assert report not in output, output[-4000:]
