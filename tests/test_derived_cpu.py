"""CPU-side checks of the derived-field operator (mdb_derived_values*, mdb_derived_buckets*, mdb_derived_apply,
mdb_derived_merge_n, mdb_derived_stats): the entry points in the built library, the header, the ctypes mirror and the
Rust binding; the layouts of mdb_derived_expr and mdb_derived_cell everywhere; mdb_derived_apply against numpy bit for
bit; mdb_derived_merge_n against the documented rule and exact arithmetic on random splits; mdb_derived_stats; and the
host side (modelardb-rs_amd/csrc/mdb_derived_host.cpp) driven by a stand-alone program, plain and under AddressSanitizer
+ UBSan (tests/derived_host)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import derived_cases as dc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "derived_host")
NAMES = ("mdb_derived_values_dev", "mdb_derived_values", "mdb_derived_buckets", "mdb_derived_buckets_dev",
         "mdb_derived_buckets_list", "mdb_derived_apply", "mdb_derived_merge_n", "mdb_derived_stats")
CELL_OFFSETS = {"count": 0, "mean": 8, "m2": 16, "min": 24, "max": 28}
EXPR_OFFSETS = {"op": 0, "flags": 4, "a": 8, "b": 12, "c": 16}
CELL = mdb.DERIVED_CELL_DTYPE


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
        # (the safe wrappers take host batches, as those of the other operators do)
        assert name.endswith("_dev") or f"sys::{name}(" in binding, name
    declared = set(re.findall(r"\b(mdb_\w+)\(", header))
    bound = set(re.findall(r"pub fn (mdb_\w+)\(", rust))
    listed = {name for name in exported if name.startswith("mdb_")}
    assert {name for name in declared | bound | listed if "derived" in name} == set(NAMES)
    assert declared == bound, declared ^ bound
    for name in NAMES:   # (other operators' CPU tests partition the symbol table by these substrings)
        assert not any(word in name for word in ("comoments", "binned", "trend", "change", "dwell", "transit", "episodes",
                                                 "integral"))


def test_layouts_and_constants_agree_everywhere():
    text = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    header = open(os.path.join(REPO_ROOT, "include", "mdb.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    for struct, mirror, size, offsets in (("mdb_derived_cell", _abi.DerivedCellC, 32, CELL_OFFSETS),
                                          ("mdb_derived_expr", _abi.DerivedExprC, 20, EXPR_OFFSETS)):
        assert ctypes.sizeof(mirror) == size
        assert [name for name, _ in mirror._fields_] == list(offsets)
        assert re.search(rf"MDB_LAYOUT_ASSERT\(sizeof\({struct}\) == {size}\)", text)
        assert re.search(rf"size_of::<{struct}>\(\) == {size}\b", rust)
        for name, offset in offsets.items():
            assert getattr(mirror, name).offset == offset, name
            assert re.search(rf"MDB_LAYOUT_ASSERT\(offsetof\({struct}, {name}\) == {offset}\)", text), name
            assert re.search(rf"offset_of!\({struct}, {name}\) == {offset}\b", rust), name
    assert CELL.itemsize == 32 and list(CELL.names) == list(CELL_OFFSETS)
    for name, offset in CELL_OFFSETS.items():
        assert CELL.fields[name][1] == offset
    rust_cell = re.search(r"pub struct mdb_derived_cell \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", rust_cell) == [("count", "i64"), ("mean", "f64"), ("m2", "f64"), ("min", "f32"), ("max", "f32")]
    rust_expr = re.search(r"pub struct mdb_derived_expr \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", rust_expr) == [("op", "u32"), ("flags", "u32"), ("a", "f32"), ("b", "f32"), ("c", "f32")]
    assert mdb.fresh_derived_cells((2, 3)).tobytes() == bytes(6 * 32)
    for name, value in mdb.DERIVED_OPS.items():
        assert re.search(rf"#define MDB_DERIVED_{name.upper()}\s+{value}u", text)
        assert re.search(rf"pub const MDB_DERIVED_{name.upper()}: u32 = {value};", rust)
        assert getattr(mdb, f"MDB_DERIVED_{name.upper()}") == value
    assert re.search(r"#define MDB_DERIVED_ABS\s+1u", text) and "pub const MDB_DERIVED_ABS: u32 = 1;" in rust
    for name in ("SHORT_ROWS", "CHUNK_ROWS"):
        value = int(re.search(rf"#define MDB_DERIVED_{name} (\d+)u", header).group(1))
        assert getattr(mdb, f"MDB_DERIVED_{name}") == value
        assert re.search(rf"pub const MDB_DERIVED_{name}: u32 = {value};", rust)
    assert mdb.MDB_DERIVED_SHORT_ROWS < mdb.MDB_DERIVED_CHUNK_ROWS and mdb.MDB_DERIVED_CHUNK_ROWS % 256 == 0


def _operands():
    """+-0, denormals, the smallest normals, infinities, NaN, values whose products and quotients are denormal or
    overflow, and random bit patterns."""
    rng = np.random.default_rng(2060)
    special = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 3e-39, 1.1754942e-38, 1.17549435e-38, 2e-38, 1e-20, -1e-20,
                        1e20, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan, 0.1, 3.0, 123456.789], dtype=np.float32)
    special = np.concatenate([special, (special.view(np.uint32)[17:18] | np.uint32(0x80000000)).view(np.float32)])  # -NaN
    random_bits = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32).view(np.float32)
    values = np.concatenate([special, random_bits])
    x, y = np.meshgrid(values, values)
    return x.reshape(-1).copy(), y.reshape(-1).copy()


@pytest.mark.parametrize("op", ["linear", "product", "ratio"])
@pytest.mark.parametrize("absolute", [False, True], ids=["plain", "abs"])
def test_apply_matches_numpy_bit_for_bit(op, absolute):
    x, y = _operands()
    denormal_results = 0
    for a, b, c in ((1.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (1.0, -1.0, -0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.1), (0.1, 1.7, -3.3),
                    (1e-20, -0.0, 0.0)):
        expr = (op, a, b, c, absolute)
        got = mdb.derived_apply(dc.expression(expr), x, y)
        expected = dc.z_of(expr, x, y)
        same = (got.view(np.uint32) == expected.view(np.uint32)) | (np.isnan(got) & np.isnan(expected))
        assert same.all(), (expr, x[~same][:5], y[~same][:5], got[~same][:5], expected[~same][:5])
        if absolute:
            assert (got.view(np.uint32) >> 31 == 0).all()   # (the sign bit of a NaN too)
        tiny = np.abs(got[np.isfinite(got)])
        denormal_results += int(((tiny > 0) & (tiny < 1.17549435e-38)).sum())
    assert denormal_results > 0
    if op == "ratio":
        z = mdb.derived_apply(dc.expression((op, 1.0, 0.0, 0.0, False)), np.float32([0.0, 1.0, -1.0]), np.float32([0.0, 0.0, 0.0]))
        assert np.isnan(z[0]) and z[1] == np.inf and z[2] == -np.inf
    if op == "linear":   # zeros follow from the formula: c = +0 turns a -0 sum into +0, c = -0 keeps it
        minus = np.float32([-0.0])
        assert mdb.derived_apply(mdb.derived_expr("linear", 1.0, 1.0, 0.0), minus, minus).view(np.uint32)[0] == 0
        assert mdb.derived_apply(mdb.derived_expr("linear", 1.0, 1.0, -0.0), minus, minus).view(np.uint32)[0] == 0x80000000


def test_bad_expressions_are_errors_and_leave_the_output_alone():
    library = mdb.load_hip_library()
    x = np.float32([1.0, 2.0])
    out = np.float32([7.0, 7.0])
    for expr, message in ((_abi.DerivedExprC(3, 0, 1.0, 1.0, 0.0), b"op"), (_abi.DerivedExprC(0, 2, 1.0, 1.0, 0.0), b"flag"),
                          (_abi.DerivedExprC(0, 0, np.nan, 1.0, 0.0), b"finite"), (_abi.DerivedExprC(1, 0, 1.0, np.inf, 0.0), b"finite"),
                          (_abi.DerivedExprC(2, 1, 1.0, 1.0, -np.inf), b"finite")):
        assert library.mdb_derived_apply(ctypes.byref(expr), x.ctypes.data, x.ctypes.data, 2, out.ctypes.data) == 1
        assert message in library.mdb_last_error()
        with pytest.raises(mdb.HipError):
            mdb.derived_apply(expr, x, x)
    assert (out == 7.0).all()
    good = _abi.DerivedExprC(0, 0, 1.0, 1.0, 0.0)
    assert library.mdb_derived_apply(None, x.ctypes.data, x.ctypes.data, 2, out.ctypes.data) == 1
    assert library.mdb_derived_apply(ctypes.byref(good), None, x.ctypes.data, 2, out.ctypes.data) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_derived_apply(ctypes.byref(good), None, None, 0, None) == 0
    with pytest.raises(ValueError):
        mdb.derived_apply(good, x, x[:1])


def test_merge_is_the_documented_rule_cell_by_cell():
    rng = np.random.default_rng(2061)
    a, b = mdb.fresh_derived_cells(5_000), mdb.fresh_derived_cells(5_000)
    for cells in (a, b):
        cells["count"] = rng.integers(0, 4, len(cells)) * rng.integers(1, 1 << 40, len(cells))
        cells["mean"] = rng.normal(0.0, 1e3, len(cells))
        cells["m2"] = rng.random(len(cells)) * 1e6
        cells["min"] = rng.normal(0.0, 1e3, len(cells)).astype(np.float32)
        cells["max"] = cells["min"] + rng.random(len(cells)).astype(np.float32) * 10
    b["min"][:50], b["max"][:50] = np.float32(3.4028235e38), np.float32(-3.4028235e38)   # (cells of NaNs only)
    assert ((a["count"] == 0) & (b["count"] > 0)).any() and ((b["count"] == 0) & (a["count"] > 0)).any()
    got = mdb.derived_merge(a.copy(), b)
    na, nb = a["count"].astype(np.float64), b["count"].astype(np.float64)
    n = (a["count"] + b["count"]).astype(np.float64)
    d = b["mean"] - a["mean"]
    with np.errstate(invalid="ignore", divide="ignore"):
        expected = mdb.fresh_derived_cells(len(a))
        expected["count"] = a["count"] + b["count"]
        expected["mean"] = a["mean"] + d * (nb / n)
        expected["m2"] = a["m2"] + b["m2"] + d * d * (na * nb / n)
        expected["min"] = np.where(b["min"] < a["min"], b["min"], a["min"])
        expected["max"] = np.where(b["max"] > a["max"], b["max"], a["max"])
    expected[a["count"] == 0] = b[a["count"] == 0]
    expected[b["count"] == 0] = a[b["count"] == 0]
    assert got.tobytes() == expected.tobytes()
    # -0.0 and +0.0 are one extreme: the one met first stays
    zeros = mdb.fresh_derived_cells(2)
    zeros[0], zeros[1] = (1, 0.0, 0.0, 0.0, 0.0), (1, -0.0, 0.0, -0.0, -0.0)
    assert np.signbit(mdb.derived_merge(zeros[:1].copy(), zeros[1:])["min"][0]) == False   # noqa: E712
    assert np.signbit(mdb.derived_merge(zeros[1:].copy(), zeros[:1])["min"][0]) == True    # noqa: E712


def test_a_fresh_cell_on_either_side_returns_the_other_sides_bytes():
    rng = np.random.default_rng(2062)
    cells = np.frombuffer(rng.bytes(32 * 2_000), dtype=CELL).copy()
    cells["count"] = np.abs(cells["count"] >> 2) + 1   # (not empty; the other members any bit pattern, NaNs among them)
    assert mdb.derived_merge(mdb.fresh_derived_cells(len(cells)), cells).tobytes() == cells.tobytes()
    assert mdb.derived_merge(cells.copy(), mdb.fresh_derived_cells(len(cells))).tobytes() == cells.tobytes()
    # count == 0: no other member is read - a cell of 0xA5 bytes with count 0 is empty
    stale = np.frombuffer(bytes([0xA5]) * (32 * len(cells)), dtype=CELL).copy()
    stale["count"] = 0
    untouched = stale.copy()
    assert mdb.derived_merge(stale, mdb.fresh_derived_cells(len(cells))).tobytes() == untouched.tobytes()
    assert mdb.derived_merge(cells.copy(), untouched).tobytes() == cells.tobytes()
    assert mdb.derived_merge(stale, cells).tobytes() == cells.tobytes()
    with pytest.raises(ValueError):
        mdb.derived_merge(cells, cells[:5])


def _assert_close(cell, z, context):
    mean, m2, low, high = dc.cell_reference(z)
    assert cell["count"] == len(z) and cell["min"] == low and cell["max"] == high, context
    assert abs(cell["mean"] - mean) <= dc.MEAN_TOLERANCE * float(np.abs(z.astype(np.float64)).max()), context
    assert abs(cell["m2"] - m2) <= dc.M2_TOLERANCE * m2, (context, cell["m2"], m2)


def test_merge_on_random_splits_meets_the_tolerance():
    """Every data set and three expressions: z cut at random places into runs (some empty), each run's cell exact, the
    runs merged one after the other, in order and shuffled; count, min and max never move."""
    rng = np.random.default_rng(2063)
    for name, (x, y) in dc.data_sets(rng, 20_000).items():
        for expr in ("absolute_difference", "product", "weighted_sum"):
            z = dc.z_of(expr, x, y)
            for n_runs in (2, 29, 400, 2858):
                cuts = np.sort(rng.integers(0, len(z) + 1, n_runs - 1))
                cells = dc.cells_of(np.split(z, cuts))
                for order in (range(1, n_runs), list(rng.permutation(np.arange(1, n_runs)))):
                    into = cells[:1].copy()
                    for k in order:
                        mdb.derived_merge(into, cells[k:k + 1])
                    _assert_close(into[0], z, (name, expr, n_runs))


def test_equal_values_keep_a_zero_m2_and_their_mean_in_any_order_of_merges():
    rng = np.random.default_rng(2064)
    for value in (np.float32(1234.567), np.float32(-1e7 - 1), np.float32(1e-40)):
        lengths = rng.integers(1, 500, 300)
        cells = mdb.fresh_derived_cells(len(lengths))
        for k, n in enumerate(lengths):
            cells[k] = (n, float(value), 0.0, value, value)
        for order in (np.arange(len(cells)), rng.permutation(len(cells))):
            into = mdb.fresh_derived_cells(1)
            for k in order:
                mdb.derived_merge(into, cells[k:k + 1])
            assert into["count"][0] == lengths.sum() and into["m2"][0] == 0.0 and into["mean"][0] == float(value)
            assert into["min"][0] == value and into["max"][0] == value


def test_stats_feed_moments_variance():
    rng = np.random.default_rng(2065)
    x, y = rng.normal(50.0, 3.0, 1000).astype(np.float32), rng.normal(-7.0, 0.2, 1000).astype(np.float32)
    z = dc.z_of("product", x, y)
    cells = dc.cells_of([z, z[:0], z[:1]])
    triple = mdb.derived_stats(cells)
    assert triple.dtype == mdb.MOMENTS_CELL_DTYPE and triple["count"].tolist() == [1000, 0, 1]
    assert triple[1].tobytes() == bytes(24)
    for ddof in (0, 1):
        variance = mdb.moments_variance(triple, ddof)
        expected = np.var(z.astype(np.float64), ddof=ddof)
        assert abs(variance[0] - expected) <= dc.M2_TOLERANCE * expected
        assert np.isnan(variance[1]) and (variance[2] == 0.0 if ddof == 0 else np.isnan(variance[2]))
    assert mdb.derived_stats(cells.reshape(3, 1)).shape == (3, 1)
    library = mdb.load_hip_library()
    out = mdb.fresh_moments_cells(3)
    assert library.mdb_derived_stats(None, 3, out.ctypes.data) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_derived_stats(cells.ctypes.data, 3, None) == 1 and b"NULL" in library.mdb_last_error()
    assert out.tobytes() == bytes(3 * 24)


def test_requests_and_expressions_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    cells = np.frombuffer(bytes([0xA5]) * (32 * 4), dtype=CELL).copy()
    before = cells.copy()
    values = np.full(8, 7.0, dtype=np.float32)
    rows = ctypes.c_uint64(99)
    lo, hi = -(1 << 63), (1 << 63) - 1
    good_expr = _abi.DerivedExprC(1, 0, 1.0, 0.0, 0.0)
    good_request = _abi.BucketRequestC(0, 100, 4, lo, hi, 1, 0)
    pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
    wrong = [(_abi.BucketRequestC(0, 100, 4, lo, hi, 1, 1), good_expr, b"which_mask"),
             (_abi.BucketRequestC(0, 0, 4, lo, hi, 1, 0), good_expr, b"width"),
             (_abi.BucketRequestC(0, 100, 4, lo, hi, 0, 0), good_expr, b"n_groups must"),
             (_abi.BucketRequestC(0, 100, (1 << 64) // 8, lo, hi, 4_000_000_000, 0), good_expr, b"overflows"),
             (good_request, _abi.DerivedExprC(3, 0, 1.0, 1.0, 0.0), b"op"),
             (good_request, _abi.DerivedExprC(0, 4, 1.0, 1.0, 0.0), b"flag"),
             (good_request, _abi.DerivedExprC(0, 0, 1.0, np.nan, 0.0), b"finite")]
    for request, expr, message in wrong:
        for call in (lambda: library.mdb_derived_buckets(fake_context, ctypes.byref(seg), ctypes.byref(seg), None,
                                                         ctypes.byref(request), ctypes.byref(expr), cells.ctypes.data),
                     lambda: library.mdb_derived_buckets_dev(fake_context, ctypes.byref(seg), ctypes.byref(seg), None,
                                                             ctypes.byref(request), ctypes.byref(expr), cells.ctypes.data),
                     lambda: library.mdb_derived_buckets_list(fake_context, pointers, 1, pointers, 1, None,
                                                              ctypes.byref(request), ctypes.byref(expr), cells.ctypes.data)):
            assert call() == 1
            assert message in library.mdb_last_error()
        if expr is not good_expr:
            for call in (library.mdb_derived_values, library.mdb_derived_values_dev):
                assert call(fake_context, ctypes.byref(seg), ctypes.byref(seg), ctypes.byref(expr), lo, hi, None,
                            values.ctypes.data, 8, ctypes.byref(rows)) == 1
                assert message in library.mdb_last_error()
    for call in (library.mdb_derived_buckets, library.mdb_derived_buckets_dev):   # a NULL y, a NULL expr
        assert call(fake_context, ctypes.byref(seg), None, None, ctypes.byref(good_request), ctypes.byref(good_expr), cells.ctypes.data) == 1
        assert b"NULL" in library.mdb_last_error()
        assert call(fake_context, ctypes.byref(seg), ctypes.byref(seg), None, ctypes.byref(good_request), None, cells.ctypes.data) == 1
        assert b"NULL" in library.mdb_last_error()
    for call in (library.mdb_derived_values, library.mdb_derived_values_dev):
        assert call(fake_context, ctypes.byref(seg), None, ctypes.byref(good_expr), lo, hi, None, values.ctypes.data, 8, ctypes.byref(rows)) == 1
        assert call(fake_context, ctypes.byref(seg), ctypes.byref(seg), ctypes.byref(good_expr), lo, hi, None, values.ctypes.data, 8, None) == 1
        # an empty range succeeds without the device
        assert call(fake_context, ctypes.byref(seg), ctypes.byref(seg), ctypes.byref(good_expr), 5, 4, None, values.ctypes.data, 8, ctypes.byref(rows)) == 0
        assert rows.value == 0
        rows.value = 99
    assert library.mdb_derived_merge_n(None, cells.ctypes.data, 1) == 1 and b"NULL" in library.mdb_last_error()
    assert cells.tobytes() == before.tobytes() and (values == 7.0).all()


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
