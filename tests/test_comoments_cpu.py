"""CPU-side checks of the covariance operator (mdb_comoments_buckets*, mdb_comoments_merge_n, mdb_comoments_moments,
mdb_comoments_finish): the entry points in the built library, the header, the ctypes mirror and the Rust binding; the
layout of mdb_comoments_cell everywhere; mdb_comoments_merge_n against exact arithmetic on random splits;
mdb_comoments_finish against numpy; and the host side (modelardb-rs_amd/csrc/mdb_comoments_host.cpp) driven by a
stand-alone program, plain and under AddressSanitizer + UBSan (tests/comoments_host)."""

import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "comoments_host")
NAMES = ("mdb_comoments_buckets", "mdb_comoments_buckets_dev", "mdb_comoments_buckets_list", "mdb_comoments_merge_n",
         "mdb_comoments_moments", "mdb_comoments_finish")
OFFSETS = {"count": 0, "mean_x": 8, "mean_y": 16, "m2_x": 24, "m2_y": 32, "c_xy": 40}
CELL = mdb.COMOMENTS_CELL_DTYPE
MEAN_TOLERANCE = 2.0 ** -44   # of the largest |v| of the field
M2_TOLERANCE = 1e-5           # of m2_ref
C_TOLERANCE = 1e-5            # of sqrt(m2x_ref * m2y_ref), the Cauchy-Schwarz bound of |c|


def test_entry_points_exported_declared_and_bound():
    library = _abi.HIP_LIBRARY_PATH
    assert os.path.exists(library), "build() first"
    exported = subprocess.run(["nm", "-D", "--defined-only", library], check=True, capture_output=True,
                              text=True).stdout.split()
    header = open(os.path.join(REPO_ROOT, "include", "mdb.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    for name in NAMES:
        assert name in exported, name
        assert re.search(rf"\bint {name}\(", header), name
        assert re.search(rf"pub fn {name}\(", rust), name
        assert name in _abi.hip_symbol_names(), name
    # the header, the Rust binding and the library name the same set of entry points
    declared = set(re.findall(r"\b(mdb_\w+)\(", header))
    bound = set(re.findall(r"pub fn (mdb_\w+)\(", rust))
    listed = {name for name in exported if name.startswith("mdb_")}
    assert {name for name in declared | bound | listed if "comoments" in name} == set(NAMES)
    assert declared == bound, declared ^ bound
    assert declared <= listed, declared - listed


def test_cell_layout_agrees_everywhere():
    assert ctypes.sizeof(_abi.ComomentsCellC) == 48 == CELL.itemsize
    assert [name for name, _ in _abi.ComomentsCellC._fields_] == list(OFFSETS) == list(CELL.names)
    text = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    assert re.search(r"MDB_LAYOUT_ASSERT\(sizeof\(mdb_comoments_cell\) == 48\)", text)
    assert re.search(r"size_of::<mdb_comoments_cell>\(\) == 48\b", rust)
    for name, offset in OFFSETS.items():
        assert getattr(_abi.ComomentsCellC, name).offset == offset == CELL.fields[name][1], name
        assert re.search(rf"MDB_LAYOUT_ASSERT\(offsetof\(mdb_comoments_cell, {name}\) == {offset}\)", text), name
        assert re.search(rf"offset_of!\(mdb_comoments_cell, {name}\) == {offset}\b", rust), name
    rust_struct = re.search(r"pub struct mdb_comoments_cell \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", rust_struct) == [("count", "i64")] + [(name, "f64") for name in list(OFFSETS)[1:]]
    c_struct = re.search(r"typedef struct mdb_comoments_cell \{(.*?)\} mdb_comoments_cell;", text, re.S).group(1)
    c_struct = re.sub(r"/\*.*?\*/", "", c_struct)
    members = [(kind, name.strip()) for kind, names in re.findall(r"(\w+)\s+([\w, ]+);", c_struct) for name in names.split(",")]
    assert members == [("int64_t", "count")] + [("double", name) for name in list(OFFSETS)[1:]]
    assert mdb.fresh_comoments_cells((2, 3)).tobytes() == bytes(6 * 48)
    for kind, value in mdb.COMOMENTS_KINDS.items():
        assert re.search(rf"#define MDB_COMOMENTS_{kind.upper()} {value}u", open(os.path.join(REPO_ROOT, "include", "mdb.h")).read())
        assert re.search(rf"pub const MDB_COMOMENTS_{kind.upper()}: u32 = {value};", rust)


def _reference(x, y):
    """(mean_x, mean_y, m2_x, m2_y, c_ref) of f32 pairs in exact arithmetic: the reference of
    tests/test_gpu_comoments.py."""
    dx = x.astype(np.float64) - float(x[0])
    dy = y.astype(np.float64) - float(y[0])
    shift_x, shift_y = math.fsum(dx) / len(dx), math.fsum(dy) / len(dy)
    rx, ry = dx - shift_x, dy - shift_y
    return float(x[0]) + shift_x, float(y[0]) + shift_y, math.fsum(rx * rx), math.fsum(ry * ry), math.fsum(rx * ry)


def _cells_of(runs):
    cells = mdb.fresh_comoments_cells(len(runs))
    for k, (x, y) in enumerate(runs):
        if len(x):
            cells[k] = (len(x),) + _reference(x, y)
    return cells


def _data_sets(rng, n):
    """Levels 0, 1e6 and 1e7 with sigma 0.5 (as the moments tests use); y correlated with, anticorrelated with and
    independent of x."""
    sets = {}
    for level in (0.0, 1.0e6, 1.0e7):
        e, f = rng.normal(0.0, 0.5, n), rng.normal(0.0, 0.5, n)
        x = (level + e).astype(np.float32)
        sets[f"level_{level:g}_correlated"] = (x, (level + 0.8 * e + 0.2 * f).astype(np.float32))
        sets[f"level_{level:g}_anticorrelated"] = (x, (level - 0.8 * e + 0.2 * f).astype(np.float32))
        sets[f"level_{level:g}_independent"] = (x, (level + f).astype(np.float32))
    return sets


def _assert_close(cell, x, y, context):
    mean_x, mean_y, m2_x, m2_y, c_ref = _reference(x, y)
    assert cell["count"] == len(x), context
    assert abs(cell["mean_x"] - mean_x) <= MEAN_TOLERANCE * float(np.abs(x.astype(np.float64)).max()), context
    assert abs(cell["mean_y"] - mean_y) <= MEAN_TOLERANCE * float(np.abs(y.astype(np.float64)).max()), context
    assert abs(cell["m2_x"] - m2_x) <= M2_TOLERANCE * m2_x, context
    assert abs(cell["m2_y"] - m2_y) <= M2_TOLERANCE * m2_y, context
    assert abs(cell["c_xy"] - c_ref) <= C_TOLERANCE * math.sqrt(m2_x * m2_y), (context, cell["c_xy"], c_ref)


def test_merge_on_random_splits_meets_the_tolerance():
    """Every data set cut at random places into runs (some empty), each run's cell exact, the runs merged one after
    the other into the first, in order and shuffled; merge(a, b) and merge(b, a) agree within the tolerances (both are
    held to the reference)."""
    rng = np.random.default_rng(2040)
    for name, (x, y) in _data_sets(rng, 20_000).items():
        for n_runs in (2, 29, 400, 2858):
            cuts = np.sort(rng.integers(0, len(x) + 1, n_runs - 1))
            runs = list(zip(np.split(x, cuts), np.split(y, cuts)))
            assert n_runs < 100 or any(len(run[0]) == 0 for run in runs)
            cells = _cells_of(runs)
            for order in (range(1, n_runs), list(rng.permutation(np.arange(1, n_runs)))):
                into = cells[:1].copy()
                for k in order:
                    mdb.comoments_merge(into, cells[k:k + 1])
                _assert_close(into[0], x, y, (name, n_runs))
        cut = int(rng.integers(1, len(x)))
        halves = _cells_of([(x[:cut], y[:cut]), (x[cut:], y[cut:])])
        _assert_close(mdb.comoments_merge(halves[:1].copy(), halves[1:])[0], x, y, (name, "a, b"))
        _assert_close(mdb.comoments_merge(halves[1:].copy(), halves[:1])[0], x, y, (name, "b, a"))


def test_merge_is_the_documented_rule_cell_by_cell():
    rng = np.random.default_rng(2041)
    a, b = mdb.fresh_comoments_cells(5_000), mdb.fresh_comoments_cells(5_000)
    for cells in (a, b):
        cells["count"] = rng.integers(0, 4, len(cells)) * rng.integers(1, 1 << 40, len(cells))
        for name in ("mean_x", "mean_y"):
            cells[name] = rng.normal(0.0, 1e3, len(cells))
        for name in ("m2_x", "m2_y"):
            cells[name] = rng.random(len(cells)) * 1e6
        cells["c_xy"] = rng.normal(0.0, 1e5, len(cells))
    assert ((a["count"] == 0) & (b["count"] > 0)).any() and ((b["count"] == 0) & (a["count"] > 0)).any()
    got = mdb.comoments_merge(a.copy(), b)
    na, nb = a["count"].astype(np.float64), b["count"].astype(np.float64)
    n = (a["count"] + b["count"]).astype(np.float64)
    dx, dy = b["mean_x"] - a["mean_x"], b["mean_y"] - a["mean_y"]
    with np.errstate(invalid="ignore", divide="ignore"):
        w = na * nb / n
        expected = mdb.fresh_comoments_cells(len(a))
        expected["count"] = a["count"] + b["count"]
        expected["mean_x"] = a["mean_x"] + dx * (nb / n)
        expected["mean_y"] = a["mean_y"] + dy * (nb / n)
        expected["m2_x"] = a["m2_x"] + b["m2_x"] + dx * dx * w
        expected["m2_y"] = a["m2_y"] + b["m2_y"] + dy * dy * w
        expected["c_xy"] = a["c_xy"] + b["c_xy"] + dx * dy * w
    expected[a["count"] == 0] = b[a["count"] == 0]
    expected[b["count"] == 0] = a[b["count"] == 0]
    assert got.tobytes() == expected.tobytes()


def test_a_fresh_cell_on_either_side_returns_the_other_sides_bytes():
    rng = np.random.default_rng(2042)
    cells = np.frombuffer(rng.bytes(48 * 2_000), dtype=CELL).copy()
    cells["count"] = np.abs(cells["count"] >> 2) + 1   # (not empty; the f64 members any bit pattern, NaNs among them)
    assert mdb.comoments_merge(mdb.fresh_comoments_cells(len(cells)), cells).tobytes() == cells.tobytes()
    assert mdb.comoments_merge(cells.copy(), mdb.fresh_comoments_cells(len(cells))).tobytes() == cells.tobytes()
    # count == 0: no other member is read - a cell of 0xA5 bytes with count 0 is empty
    stale = np.frombuffer(bytes([0xA5]) * (48 * len(cells)), dtype=CELL).copy()
    stale["count"] = 0
    untouched = stale.copy()
    assert mdb.comoments_merge(stale, mdb.fresh_comoments_cells(len(cells))).tobytes() == untouched.tobytes()
    assert mdb.comoments_merge(stale, cells).tobytes() == cells.tobytes()
    with pytest.raises(ValueError):
        mdb.comoments_merge(cells, cells[:5])


def test_identical_fields_keep_the_same_bytes_through_any_sequence_of_merges():
    """x == y element for element: m2_x, m2_y and c_xy have the same bytes after any sequence of merges, and
    comoments_finish(CORR) is exactly 1.0 wherever m2 > 0. The cells of the runs come from the library's own run
    arithmetic where a run is one point (count 1, the value, zeros) and from the reference otherwise."""
    rng = np.random.default_rng(2043)
    for level in (0.0, 1.0e6, 1.0e7):
        x = (level + rng.normal(0.0, 0.5, 5_000)).astype(np.float32)
        for n_runs in (2, 50, 1_000, 5_000):
            cuts = np.sort(rng.choice(np.arange(1, len(x)), n_runs - 1, replace=False))
            runs = np.split(x, cuts)
            cells = mdb.fresh_comoments_cells(len(runs))
            for k, run in enumerate(runs):
                mean, _, m2, _, _ = _reference(run, run)
                cells[k] = (len(run), mean, mean, m2, m2, m2)
            for order in (np.arange(len(runs)), rng.permutation(len(runs))):
                # a chain, and a tree of pairs
                chain = mdb.fresh_comoments_cells(1)
                for k in order:
                    mdb.comoments_merge(chain, cells[k:k + 1])
                level_cells = cells[order].copy()
                while len(level_cells) > 1:
                    half = len(level_cells) // 2
                    merged = mdb.comoments_merge(level_cells[:half].copy(), level_cells[half:2 * half])
                    level_cells = np.concatenate([merged, level_cells[2 * half:]])
                for cell in (chain[0], level_cells[0]):
                    assert cell["count"] == len(x)
                    assert cell["m2_x"].tobytes() == cell["m2_y"].tobytes() == cell["c_xy"].tobytes()
                    assert cell["mean_x"].tobytes() == cell["mean_y"].tobytes() and cell["m2_x"] > 0.0
                assert mdb.comoments_finish(chain, "corr")[0] == 1.0
                assert mdb.comoments_finish(level_cells[:1], mdb.COMOMENTS_KINDS["corr"])[0] == 1.0


def test_a_constant_field_has_no_covariance_in_any_order_of_merges():
    rng = np.random.default_rng(2044)
    x = (1.0e6 + rng.normal(0.0, 0.5, 4_000)).astype(np.float32)
    y = np.full(len(x), 1234.567, dtype=np.float32)
    cuts = np.sort(rng.integers(1, len(x), 300))
    for first, second, constant in ((x, y, "y"), (y, x, "x")):
        cells = _cells_of(list(zip(np.split(first, cuts), np.split(second, cuts))))
        for order in (np.arange(len(cells)), rng.permutation(len(cells))):
            into = mdb.fresh_comoments_cells(1)
            for k in order:
                mdb.comoments_merge(into, cells[k:k + 1])
            assert into["c_xy"][0] == 0.0 and into["m2_" + constant][0] == 0.0
            assert into["mean_" + constant][0] == float(y[0]) and into["count"][0] == len(x)
            for kind in ("corr", "regr_r2"):
                assert np.isnan(mdb.comoments_finish(into, kind)[0])
            assert mdb.comoments_finish(into, "covar_samp")[0] == 0.0


def test_finish_for_all_six_kinds_against_numpy():
    rng = np.random.default_rng(2045)
    x = rng.normal(50.0, 3.0, 1000).astype(np.float32)
    y = (0.7 * x + rng.normal(0.0, 1.0, 1000)).astype(np.float32)
    cell = _cells_of([(x, y)])
    wide_x, wide_y = x.astype(np.float64), y.astype(np.float64)
    slope, intercept = np.polyfit(wide_x, wide_y, 1)   # (y on x: x is the independent variable)
    corr = np.corrcoef(wide_x, wide_y)[0, 1]
    for kind, value in (("covar_pop", np.cov(wide_x, wide_y, ddof=0)[0, 1]), ("covar_samp", np.cov(wide_x, wide_y, ddof=1)[0, 1]),
                        ("corr", corr), ("regr_slope", slope), ("regr_intercept", intercept), ("regr_r2", corr * corr)):
        got = mdb.comoments_finish(cell, kind)[0]
        assert abs(got - value) <= 1e-9 * max(abs(value), 1.0), (kind, got, value)
    # the NaN cases: n = 0, n = 1, either m2 = 0
    cells = mdb.fresh_comoments_cells(5)
    cells[1] = (1, 5.0, 6.0, 0.0, 0.0, 0.0)
    cells[2] = (4, 1.0, 10.0, 8.0, 2.0, -3.0)
    cells[3] = (4, 1.0, 10.0, 0.0, 2.0, 0.0)
    cells[4] = (4, 1.0, 10.0, 8.0, 0.0, 0.0)
    expected = {"covar_pop": [None, 0.0, -0.75, 0.0, 0.0], "covar_samp": [None, None, -1.0, 0.0, 0.0],
                "corr": [None, None, -0.75, None, None], "regr_slope": [None, None, -0.375, None, 0.0],
                "regr_intercept": [None, None, 10.375, None, 10.0], "regr_r2": [None, None, 0.5625, None, None]}
    for kind, values in expected.items():
        got = mdb.comoments_finish(cells, kind)
        for k, value in enumerate(values):
            assert np.isnan(got[k]) if value is None else got[k] == value, (kind, k, got[k])
    assert mdb.comoments_finish(cells.reshape(5, 1), "corr").shape == (5, 1)
    library = mdb.load_hip_library()
    out = np.full(5, 77.0)
    for kind in (6, 7, 1 << 31):
        with pytest.raises(mdb.HipError, match="kind"):
            mdb.comoments_finish(cells, kind)
        assert library.mdb_comoments_finish(cells.ctypes.data, 5, kind, out.ctypes.data) == 1 and (out == 77.0).all()
    assert library.mdb_comoments_finish(None, 1, 0, out.ctypes.data) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_comoments_finish(cells.ctypes.data, 1, 0, None) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_comoments_finish(None, 0, 0, None) == 0


def test_moments_of_either_field_give_numpys_variance():
    rng = np.random.default_rng(2046)
    x = rng.normal(50.0, 3.0, 1000).astype(np.float32)
    y = rng.normal(-7.0, 0.2, 1000).astype(np.float32)
    cells = _cells_of([(x, y), (x[:0], y[:0]), (x[:1], y[:1])])
    for which, values in ((0, x), (1, y), ("x", x), ("y", y)):
        triple = mdb.comoments_moments(cells, which)
        assert triple.dtype == mdb.MOMENTS_CELL_DTYPE and triple["count"].tolist() == [1000, 0, 1]
        assert triple[1].tobytes() == bytes(24)
        for ddof in (0, 1):
            variance = mdb.moments_variance(triple, ddof)
            expected = np.var(values.astype(np.float64), ddof=ddof)
            assert abs(variance[0] - expected) <= M2_TOLERANCE * expected
            assert np.isnan(variance[1]) and (variance[2] == 0.0 if ddof == 0 else np.isnan(variance[2]))
    library = mdb.load_hip_library()
    out = mdb.fresh_moments_cells(3)
    assert library.mdb_comoments_moments(cells.ctypes.data, 3, 2, out.ctypes.data) == 1 and b"which" in library.mdb_last_error()
    assert library.mdb_comoments_moments(None, 3, 0, out.ctypes.data) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_comoments_moments(cells.ctypes.data, 3, 0, None) == 1 and b"NULL" in library.mdb_last_error()
    assert out.tobytes() == bytes(3 * 24)


def test_requests_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    cells = np.frombuffer(bytes([0xA5]) * (48 * 4), dtype=CELL).copy()
    before = cells.copy()
    lo, hi = -(1 << 63), (1 << 63) - 1
    for request, message in ((_abi.BucketRequestC(0, 100, 4, lo, hi, 1, 1), b"which_mask"),
                             (_abi.BucketRequestC(0, 0, 4, lo, hi, 1, 0), b"width"),
                             (_abi.BucketRequestC(0, 100, 4, lo, hi, 0, 0), b"n_groups must"),
                             (_abi.BucketRequestC(0, 100, (1 << 64) // 8, lo, hi, 4_000_000_000, 0), b"overflows")):
        pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
        for call in (lambda: library.mdb_comoments_buckets(fake_context, ctypes.byref(seg), ctypes.byref(seg), None,
                                                           ctypes.byref(request), cells.ctypes.data),
                     lambda: library.mdb_comoments_buckets_dev(fake_context, ctypes.byref(seg), ctypes.byref(seg), None,
                                                               ctypes.byref(request), cells.ctypes.data),
                     lambda: library.mdb_comoments_buckets_list(fake_context, pointers, 1, pointers, 1, None,
                                                                ctypes.byref(request), cells.ctypes.data)):
            assert call() == 1
            assert message in library.mdb_last_error()
        assert cells.tobytes() == before.tobytes()
    request = _abi.BucketRequestC(0, 100, 4, lo, hi, 1, 0)
    assert library.mdb_comoments_buckets(None, None, None, None, None, None) == 1 and b"NULL" in library.mdb_last_error()
    for call in (library.mdb_comoments_buckets, library.mdb_comoments_buckets_dev):   # a NULL y
        assert call(fake_context, ctypes.byref(seg), None, None, ctypes.byref(request), cells.ctypes.data) == 1
        assert b"NULL" in library.mdb_last_error()
    assert library.mdb_comoments_buckets_list(fake_context, pointers, 1, None, 1, None, ctypes.byref(request), cells.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    assert library.mdb_comoments_merge_n(None, cells.ctypes.data, 1) == 1 and b"NULL" in library.mdb_last_error()
    assert cells.tobytes() == before.tobytes()


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
