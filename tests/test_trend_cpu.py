"""CPU-side checks of the trend operator (mdb_trend_buckets*): the entry points in the built library, the header, the
ctypes mirror and the Rust binding; the request checks, made before the device is used; and the host side
(modelardb-rs_amd/csrc/mdb_trend_host.cpp, the closed forms of mdb_trend.hpp) driven by a stand-alone program, plain
and under AddressSanitizer + UBSan (tests/trend_host)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "trend_host")
NAMES = ("mdb_trend_buckets", "mdb_trend_buckets_dev", "mdb_trend_buckets_list")
CELL = mdb.COMOMENTS_CELL_DTYPE


def test_entry_points_exported_declared_and_bound():
    library = _abi.HIP_LIBRARY_PATH
    assert os.path.exists(library), "build() first"
    exported = subprocess.run(["nm", "-D", "--defined-only", library], check=True, capture_output=True,
                              text=True).stdout.split()
    header = open(os.path.join(REPO_ROOT, "include", "mdb.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    wrappers = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in exported, name
        assert re.search(rf"\bint {name}\(", header), name
        assert re.search(rf"pub fn {name}\(", rust), name
        assert name in _abi.hip_symbol_names(), name
    declared = set(re.findall(r"\b(mdb_\w+)\(", header))
    listed = {name for name in exported if name.startswith("mdb_")}
    assert {name for name in declared | listed if "trend" in name} == set(NAMES)
    for method in ("trend_buckets", "trend_buckets_list"):
        assert re.search(rf"pub fn {method}\(", wrappers), method
    for method in ("trend_buckets", "trend_buckets_list", "trend_buckets_dev", "trend"):
        assert callable(getattr(mdb.Context, method)), method
    # the cells are mdb_comoments_cell: the merge and the statistics of the covariance operator apply as they are
    for name in NAMES:
        declaration = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        assert "mdb_comoments_cell *inout" in declaration and "const mdb_bucket_request *request" in declaration


def test_requests_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    cells = np.frombuffer(bytes([0xA5]) * (48 * 4), dtype=CELL).copy()
    before = cells.copy()
    lo, hi = -(1 << 63), (1 << 63) - 1
    pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
    groups = (ctypes.c_void_p * 1)(None)
    for request, message in ((_abi.BucketRequestC(0, 100, 4, lo, hi, 1, 1), b"which_mask must be 0 for mdb_trend_buckets"),
                             (_abi.BucketRequestC(0, 0, 4, lo, hi, 1, 0), b"width"),
                             (_abi.BucketRequestC(0, -3, 4, lo, hi, 1, 0), b"width"),
                             (_abi.BucketRequestC(0, 100, 4, lo, hi, 0, 0), b"n_groups must"),
                             (_abi.BucketRequestC(0, 100, (1 << 64) // 8, lo, hi, 4_000_000_000, 0), b"overflows")):
        for call in (lambda: library.mdb_trend_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(request),
                                                       cells.ctypes.data),
                     lambda: library.mdb_trend_buckets_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(request),
                                                           cells.ctypes.data),
                     lambda: library.mdb_trend_buckets_list(fake_context, pointers, groups, 1, ctypes.byref(request),
                                                            cells.ctypes.data)):
            assert call() == 1
            assert message in library.mdb_last_error()
        assert cells.tobytes() == before.tobytes()
    request = _abi.BucketRequestC(0, 100, 4, lo, hi, 1, 0)
    assert library.mdb_trend_buckets(None, None, None, None, None) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_trend_buckets_dev(fake_context, None, None, ctypes.byref(request), cells.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    assert library.mdb_trend_buckets_list(fake_context, None, None, 1, ctypes.byref(request), cells.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    # nothing to do: success without a context that could be used
    no_buckets = _abi.BucketRequestC(0, 100, 0, lo, hi, 1, 0)
    assert library.mdb_trend_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(no_buckets), cells.ctypes.data) == 0
    assert library.mdb_trend_buckets_list(fake_context, pointers, groups, 0, ctypes.byref(request), cells.ctypes.data) == 0
    assert cells.tobytes() == before.tobytes()


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
