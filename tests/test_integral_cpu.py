"""CPU-side checks of the time-weighted operator (mdb_integral_buckets*): the entry points in the built library, the
header, the ctypes mirror and the Rust binding; the request checks, made before the device is used; and the host side
(modelardb-rs_amd/csrc/mdb_integral_host.cpp, the interval arithmetic of mdb_integral.hpp) driven by a stand-alone
program, plain and under AddressSanitizer + UBSan (tests/integral_host)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "integral_host")
NAMES = ("mdb_integral_buckets", "mdb_integral_buckets_dev", "mdb_integral_buckets_list", "mdb_integral_merge_n",
         "mdb_integral_average")
CELL = mdb.INTEGRAL_CELL_DTYPE
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


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
    assert {name for name in declared | listed if "integral" in name} == set(NAMES)
    for method in ("integral_buckets", "integral_buckets_list", "integral_merge", "integral_average"):
        assert re.search(rf"pub fn {method}\(", wrappers), method
    for method in ("integral_buckets", "integral_buckets_list", "integral_buckets_dev", "integral"):
        assert callable(getattr(mdb.Context, method)), method
    assert callable(mdb.integral_merge) and callable(mdb.integral_average)
    # the layouts: the header's, the ctypes mirror's, numpy's and the Rust binding's
    assert "typedef struct mdb_integral_cell" in layout and "typedef struct mdb_integral_request" in layout
    assert re.search(r"#define MDB_INTEGRAL_LINEAR 0u", layout) and re.search(r"#define MDB_INTEGRAL_STEP\s+1u", layout)
    assert (mdb.MDB_INTEGRAL_LINEAR, mdb.MDB_INTEGRAL_STEP) == (0, 1)
    assert "pub const MDB_INTEGRAL_LINEAR: u32 = 0;" in rust and "pub const MDB_INTEGRAL_STEP: u32 = 1;" in rust
    assert ctypes.sizeof(_abi.IntegralCellC) == CELL.itemsize == 16 and CELL.fields["integral"][1] == 8
    assert _abi.IntegralCellC.integral.offset == 8
    request = _abi.IntegralRequestC
    assert ctypes.sizeof(request) == 64
    assert (request.max_gap.offset, request.method.offset, request.flags.offset) == (48, 56, 60)
    for text in ("sizeof(mdb_integral_cell) == 16", "sizeof(mdb_integral_request) == 64",
                 "offsetof(mdb_integral_request, max_gap) == 48", "offsetof(mdb_integral_request, method) == 56"):
        assert text in layout, text
    for text in ("size_of::<mdb_integral_cell>() == 16", "size_of::<mdb_integral_request>() == 64",
                 "offset_of!(mdb_integral_request, max_gap) == 48", "offset_of!(mdb_integral_request, method) == 56"):
        assert text in rust, text


def _request(origin=0, width=100, n_buckets=4, t_lo=I64_MIN, t_hi=I64_MAX, n_groups=1, which_mask=0, max_gap=I64_MAX,
             method=0, flags=0):
    request = _abi.IntegralRequestC()
    request.buckets = _abi.BucketRequestC(origin, width, n_buckets, t_lo, t_hi, n_groups, which_mask)
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
    for request, message in ((_request(which_mask=1), b"which_mask must be 0 for mdb_integral_buckets"),
                             (_request(width=0), b"width"),
                             (_request(width=-3), b"width"),
                             (_request(n_groups=0), b"n_groups must"),
                             (_request(n_buckets=(1 << 64) // 8, n_groups=4_000_000_000), b"overflows"),
                             (_request(t_lo=0), b"time range"),
                             (_request(t_hi=I64_MAX - 1), b"time range"),
                             (_request(method=2), b"method"),
                             (_request(flags=1), b"flags"),
                             (_request(max_gap=-1), b"max_gap")):
        for call in (lambda: library.mdb_integral_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(request),
                                                          cells.ctypes.data),
                     lambda: library.mdb_integral_buckets_dev(fake_context, ctypes.byref(seg), None,
                                                              ctypes.byref(request), cells.ctypes.data),
                     lambda: library.mdb_integral_buckets_list(fake_context, pointers, groups, 1, ctypes.byref(request),
                                                               cells.ctypes.data)):
            assert call() == 1
            assert message in library.mdb_last_error(), (message, library.mdb_last_error())
        assert cells.tobytes() == before.tobytes()
    request = _request()
    assert library.mdb_integral_buckets(None, None, None, None, None) == 1 and b"NULL" in library.mdb_last_error()
    for arguments in ((None, ctypes.byref(seg), None, ctypes.byref(request), cells.ctypes.data),
                      (fake_context, None, None, ctypes.byref(request), cells.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, None, cells.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, ctypes.byref(request), None)):
        assert library.mdb_integral_buckets(*arguments) == 1 and b"NULL" in library.mdb_last_error()
        assert library.mdb_integral_buckets_dev(*arguments) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_integral_buckets_list(fake_context, None, None, 1, ctypes.byref(request), cells.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    # nothing to do: success without a context that could be used
    no_buckets = _request(n_buckets=0)
    assert library.mdb_integral_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(no_buckets), cells.ctypes.data) == 0
    assert library.mdb_integral_buckets_list(fake_context, pointers, groups, 0, ctypes.byref(request), cells.ctypes.data) == 0
    assert cells.tobytes() == before.tobytes()


def test_merge_and_average_on_the_host():
    cells = mdb.fresh_integral_cells(4)
    assert cells.tobytes() == bytes(64)
    cells["duration"] = [0, 4, 10, 3]
    cells["integral"] = [0.0, 10.0, -2.5, np.inf]
    average = mdb.integral_average(cells)
    assert np.isnan(average[0]) and average[1] == 2.5 and average[2] == -0.25 and np.isinf(average[3])
    other = mdb.fresh_integral_cells(4)
    other["duration"] = [7, 0, 1, (1 << 64) - 4]
    other["integral"] = [1.5, 0.0, 2.5, np.nan]
    merged = mdb.integral_merge(cells.copy(), other)
    assert merged["duration"].tolist() == [7, 4, 11, (1 << 64) - 1]
    assert merged["integral"][:3].tolist() == [1.5, 10.0, 0.0] and np.isnan(merged["integral"][3])
    assert mdb.integral_average(cells.reshape(2, 2)).shape == (2, 2)
    with pytest.raises(ValueError):
        mdb.integral_merge(cells, other[:3])
    with pytest.raises(ValueError):
        mdb.integral_average(np.zeros(3))


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
