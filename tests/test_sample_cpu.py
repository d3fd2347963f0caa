"""CPU-side checks of the sampling operator (mdb_sample_at*): the entry points in the built library, the header, the
ctypes mirror and the Rust binding; the request checks, made before the device is used; merge and values on the host;
the reference's own cross-checks (tests/sample_cases.py against the oracle's grid); and the host side
(modelardb-rs_amd/csrc/mdb_sample_host.cpp, the plain C++ part of mdb_sample.hpp) driven by a stand-alone program,
plain and under AddressSanitizer + UBSan (tests/sample_host)."""

import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import comoments_cases as cc
import sample_cases as sc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "sample_host")
NAMES = ("mdb_sample_at", "mdb_sample_at_dev", "mdb_sample_at_list", "mdb_sample_merge_n", "mdb_sample_values")
CELL = mdb.SAMPLE_CELL_DTYPE
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INTERVAL = cc.INTERVAL


def test_entry_points_exported_declared_and_bound():
    library = _abi.HIP_LIBRARY_PATH
    assert os.path.exists(library), "build() first"
    exported = subprocess.run(["nm", "-D", "--defined-only", library], check=True, capture_output=True,
                              text=True).stdout.split()
    header = open(os.path.join(REPO_ROOT, "include", "mdb.h")).read()
    layout = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    wrappers = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in exported, name
        assert re.search(rf"\bint {name}\(", header), name
        assert re.search(rf"pub fn {name}\(", rust), name
        assert name in _abi.hip_symbol_names(), name
    declared = set(re.findall(r"\b(mdb_\w+)\(", header))
    listed = {name for name in exported if name.startswith("mdb_")}
    assert {name for name in declared | listed if name.startswith("mdb_sample")} == set(NAMES)
    for method in ("sample_at", "sample_at_list", "sample_merge", "sample_values"):
        assert re.search(rf"pub fn {method}\(", wrappers), method
    for method in ("sample_at", "sample_at_list", "sample_at_dev"):
        assert callable(getattr(mdb.Context, method)), method
    assert callable(mdb.sample_merge) and callable(mdb.sample_values) and callable(mdb.fresh_sample_cells)
    # the layouts: the header's, the ctypes mirror's, numpy's and the Rust binding's
    assert "typedef struct mdb_sample_cell" in layout and "typedef struct mdb_sample_request" in layout
    for name, value in (("LINEAR", 0), ("STEP", 1), ("EXACT", 2)):
        assert re.search(rf"#define MDB_SAMPLE_{name}\s+{value}u", layout), name
        assert getattr(mdb, f"MDB_SAMPLE_{name}") == value
        assert f"pub const MDB_SAMPLE_{name}: u32 = {value};" in rust
    assert ctypes.sizeof(_abi.SampleCellC) == CELL.itemsize == 16
    assert (CELL.fields["count"][1], CELL.fields["sum"][1]) == (0, 8)
    assert (_abi.SampleCellC.count.offset, _abi.SampleCellC.sum.offset) == (0, 8)
    request = _abi.SampleRequestC
    assert ctypes.sizeof(request) == 64
    assert (request.instants.offset, request.max_gap.offset, request.method.offset, request.flags.offset) == (0, 48, 56, 60)
    for text in ("sizeof(mdb_sample_cell) == 16", "offsetof(mdb_sample_cell, count) == 0",
                 "offsetof(mdb_sample_cell, sum) == 8", "sizeof(mdb_sample_request) == 64",
                 "offsetof(mdb_sample_request, instants) == 0", "offsetof(mdb_sample_request, max_gap) == 48",
                 "offsetof(mdb_sample_request, method) == 56", "offsetof(mdb_sample_request, flags) == 60"):
        assert text in layout, text
    for text in ("size_of::<mdb_sample_cell>() == 16", "size_of::<mdb_sample_request>() == 64",
                 "offset_of!(mdb_sample_request, max_gap) == 48", "offset_of!(mdb_sample_request, method) == 56"):
        assert text in rust, text


def _request(origin=0, width=100, n_instants=4, t_lo=I64_MIN, t_hi=I64_MAX, n_groups=1, which_mask=0, max_gap=I64_MAX,
             method=0, flags=0):
    request = _abi.SampleRequestC()
    request.instants = _abi.BucketRequestC(origin, width, n_instants, t_lo, t_hi, n_groups, which_mask)
    request.max_gap, request.method, request.flags = max_gap, method, flags
    return request


def test_requests_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    cells = np.frombuffer(bytes([0xA5]) * (16 * 4), dtype=CELL).copy()
    before = cells.copy()
    pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
    groups = (ctypes.c_void_p * 1)(None)
    for request, message in ((_request(which_mask=1), b"which_mask must be 0 for mdb_sample_at"),
                             (_request(width=0), b"width"),
                             (_request(width=-3), b"width"),
                             (_request(n_groups=0), b"n_groups must"),
                             (_request(n_instants=(1 << 64) // 8, n_groups=4_000_000_000), b"overflows"),
                             (_request(t_lo=0), b"time range"),
                             (_request(t_hi=I64_MAX - 1), b"time range"),
                             (_request(method=3), b"method"),
                             (_request(flags=1), b"flags"),
                             (_request(max_gap=-1), b"max_gap")):
        for call in (lambda: library.mdb_sample_at(fake_context, ctypes.byref(seg), None, ctypes.byref(request),
                                                   cells.ctypes.data),
                     lambda: library.mdb_sample_at_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(request),
                                                       cells.ctypes.data),
                     lambda: library.mdb_sample_at_list(fake_context, pointers, groups, 1, ctypes.byref(request),
                                                        cells.ctypes.data)):
            assert call() == 1
            assert message in library.mdb_last_error(), (message, library.mdb_last_error())
        assert cells.tobytes() == before.tobytes()
    request = _request()
    assert library.mdb_sample_at(None, None, None, None, None) == 1 and b"NULL" in library.mdb_last_error()
    for arguments in ((None, ctypes.byref(seg), None, ctypes.byref(request), cells.ctypes.data),
                      (fake_context, None, None, ctypes.byref(request), cells.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, None, cells.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, ctypes.byref(request), None)):
        assert library.mdb_sample_at(*arguments) == 1 and b"NULL" in library.mdb_last_error()
        assert library.mdb_sample_at_dev(*arguments) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_sample_at_list(fake_context, None, None, 1, ctypes.byref(request), cells.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    # nothing to do: success without a context that could be used
    no_instants = _request(n_instants=0)
    assert library.mdb_sample_at(fake_context, ctypes.byref(seg), None, ctypes.byref(no_instants), cells.ctypes.data) == 0
    assert library.mdb_sample_at_list(fake_context, pointers, groups, 0, ctypes.byref(request), cells.ctypes.data) == 0
    assert cells.tobytes() == before.tobytes()


def test_merge_and_values_on_the_host():
    cells = mdb.fresh_sample_cells(4)
    assert cells.tobytes() == bytes(64)
    cells["count"] = [0, 4, 10, 3]
    cells["sum"] = [0.0, 10.0, -2.5, np.inf]
    values = mdb.sample_values(cells)
    assert np.isnan(values[0]) and values[1] == 2.5 and values[2] == -0.25 and np.isinf(values[3])
    other = mdb.fresh_sample_cells(4)
    other["count"] = [1, 0, 1, (1 << 64) - 4]
    other["sum"] = [-0.0, 0.0, 2.5, np.nan]
    merged = mdb.sample_merge(cells.copy(), other)
    assert merged["count"].tolist() == [1, 4, 11, (1 << 64) - 1]
    # a cell that has received nothing takes the other whole: the -0.0 survives; the others are added
    assert merged["sum"][:1].tobytes() == np.array([-0.0]).tobytes()
    assert merged["sum"][1:3].tolist() == [10.0, 0.0] and np.isnan(merged["sum"][3])
    assert mdb.sample_merge(other.copy(), mdb.fresh_sample_cells(4)).tobytes() == other.tobytes()
    assert mdb.sample_values(cells.reshape(2, 2)).shape == (2, 2)
    with pytest.raises(ValueError):
        mdb.sample_merge(cells, other[:3])
    with pytest.raises(ValueError):
        mdb.sample_values(np.zeros(3))


def test_the_reference_on_a_series_own_grid_is_the_grid():
    """A regular single-series field sampled on its own grid: under all three methods every instant holds exactly one
    contribution, the row's value."""
    field = cc.Field([cc.main_table()[0].parts[0]])
    first, last = int(field.ts.min()), int(field.ts.max())
    assert (np.diff(field.ts) == INTERVAL).all()
    n = (last - first) // INTERVAL + 1
    assert n == len(field.ts)
    for method, name in sc.METHODS:
        expected = sc.oracle(field, None, 1, first, INTERVAL, n, method)
        assert (expected["count"] == 1).all() and expected["finite"].all(), name
        assert [float(s) for s in expected["sum"][0]] == field.values.astype(np.float64).tolist(), name
        assert np.array_equal(sc.values_of(expected)[0].astype(np.float32), field.values), name


def test_the_reference_methods_agree_where_they_must():
    """STEP and LINEAR agree on every instant that lies on a row and nowhere between rows (their contributions there
    are rows only); EXACT's count is <= the others' everywhere and equal on the instants no interval contains."""
    field = cc.main_table()[1]
    first, last = int(field.ts.min()), int(field.ts.max())
    origin, width = first - 30, 70
    n = (last - origin) // width + 2
    linear, step, exact = (sc.oracle(field, field.groups, 4, origin, width, n, method) for method, _ in sc.METHODS)
    np.testing.assert_array_equal(linear["count"], step["count"])
    assert (exact["count"] <= linear["count"]).all() and (exact["count"] < linear["count"]).any()
    on_row_only = (exact["count"] == linear["count"]) & (exact["count"] > 0)
    assert on_row_only.any()
    assert (linear["sum"][on_row_only] == exact["sum"][on_row_only]).all()
    assert (step["sum"][on_row_only] == exact["sum"][on_row_only]).all()
    # an instant between two rows of different values: LINEAR lies strictly between them, STEP is the earlier row
    between = (exact["count"] == 0) & (linear["count"] == 1)
    assert between.any()
    rows = {(int(g), int(t)): float(v) for g, t, v in zip(field.groups[field.segment], field.ts, field.values)}
    checked = 0
    for group, k in zip(*np.nonzero(between)):
        at = origin + int(k) * width
        times = field.ts[field.groups[field.segment] == group]
        before, after = int(times[times < at].max()), int(times[times > at].min())
        v0, v1 = rows[(group, before)], rows[(group, after)]
        assert step["sum"][group, k] == Fraction(v0)
        assert min(v0, v1) <= linear["sum"][group, k] <= max(v0, v1)
        checked += 1
        if checked == 200:
            break
    # a gap rule below the sampling interval of a regular series leaves rows only
    regular = cc.Field([cc.main_table()[0].parts[0]])
    args = (int(regular.ts.min()) - 30, 70, 300)
    for method, _ in sc.METHODS[:2]:
        cut = sc.oracle(regular, None, 1, *args, method, max_gap=INTERVAL - 1)
        np.testing.assert_array_equal(cut["count"], sc.oracle(regular, None, 1, *args, sc.EXACT)["count"])


@pytest.fixture(scope="module")
def built():
    done = subprocess.run(["make", "-C", HERE, "all"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "warning" not in done.stdout + done.stderr, done.stdout + done.stderr


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
