"""CPU-side checks of the per-bucket histograms and quantiles (mdb_hist_buckets*, mdb_quantile_buckets*): the entry points
in the built library, the header, the ctypes mirror and the Rust binding; the two constants everywhere; the checks a
request gets before the device is used; and the selection step host and device share
(modelardb-rs_amd/csrc/mdb_select.hpp) driven by a stand-alone program, plain and under AddressSanitizer + UBSan
(tests/hist_buckets_host). No sanitizer runs on code loaded into Python."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "hist_buckets_host")
NAMES = ("mdb_hist_buckets", "mdb_hist_buckets_dev", "mdb_hist_buckets_list", "mdb_quantile_buckets",
         "mdb_quantile_buckets_dev")


def _read(*parts):
    with open(os.path.join(REPO_ROOT, *parts)) as handle:
        return handle.read()


def test_entry_points_exported_declared_and_bound():
    library = _abi.HIP_LIBRARY_PATH
    assert os.path.exists(library), "build() first"
    exported = subprocess.run(["nm", "-D", "--defined-only", library], check=True, capture_output=True,
                              text=True).stdout.split()
    header, rust = _read("include", "mdb.h"), _read("rust", "modelardb_hip", "src", "sys.rs")
    for name in NAMES:
        assert name in exported, name
        assert re.search(rf"\bint {name}\(", header), name
        assert re.search(rf"pub fn {name}\(", rust), name
        assert name in _abi.hip_symbol_names(), name
    for method in ("hist_buckets", "hist_buckets_list", "hist_buckets_dev", "quantile_buckets", "quantile_buckets_dev"):
        assert callable(getattr(mdb.Context, method)), method


def test_the_constants_agree_everywhere():
    header, rust = _read("include", "mdb.h"), _read("rust", "modelardb_hip", "src", "sys.rs")
    select = _read("modelardb-rs_amd", "csrc", "mdb_select.hpp")
    kernels = _read("modelardb-rs_amd", "csrc", "mdb_hist_buckets.hip")
    for name, value in (("MDB_QUANTILE_BUCKETS_MAX_Q", 4), ("MDB_QUANTILE_BUCKETS_PASSES", 4)):
        assert int(re.search(rf"#define {name} (\d+)u\b", header).group(1)) == value, name
        assert int(re.search(rf"pub const {name}: u32 = (\d+);", rust).group(1)) == value, name
        assert getattr(_abi, name) == value == getattr(mdb, name), name
    assert _abi.MDB_QUANTILE_BUCKETS_PASSES <= 4, "at most 4 passes over the batch, whatever the number of cells"
    # the passes the code runs ARE the header's: digits of 8 bits over 32-bit keys, asserted where the kernels are built
    assert re.search(r"SELECT_DIGIT_BITS = 8;", select) and re.search(r"SELECT_PASSES = 32 / SELECT_DIGIT_BITS;", select)
    assert "static_assert(SELECT_PASSES == MDB_QUANTILE_BUCKETS_PASSES" in kernels


def test_requests_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
    counts = np.frombuffer(bytes([0xA5]) * (8 * 4 * 3), dtype=np.uint64).copy()
    lo_out = np.frombuffer(bytes([0xA5]) * (4 * 4 * 4), dtype=np.float32).copy()
    hi_out, n_points = lo_out.copy(), counts.copy()
    before = [a.tobytes() for a in (counts, lo_out, hi_out, n_points)]
    edges, q = np.array([1.0, 2.0], dtype=np.float32), np.array([0.5], dtype=np.float64)
    lo, hi = -(1 << 63), (1 << 63) - 1
    good = _abi.BucketRequestC(0, 100, 4, lo, hi, 1, 0)

    kept = []

    def hist_calls(request, edge_array, n_edges):
        kept.append(edge_array)   # (the calls are made later: the array must outlive this loop)
        e = None if edge_array is None else edge_array.ctypes.data
        return (lambda: library.mdb_hist_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(request), e, n_edges, counts.ctypes.data),
                lambda: library.mdb_hist_buckets_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(request), e, n_edges, counts.ctypes.data),
                lambda: library.mdb_hist_buckets_list(fake_context, pointers, None, 1, ctypes.byref(request), e, n_edges, counts.ctypes.data))

    def quantile_calls(request, q_array, n_q):
        return (lambda: library.mdb_quantile_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(request), q_array.ctypes.data, n_q,
                                                     lo_out.ctypes.data, hi_out.ctypes.data, n_points.ctypes.data),
                lambda: library.mdb_quantile_buckets_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(request), q_array.ctypes.data,
                                                         n_q, lo_out.ctypes.data, hi_out.ctypes.data, n_points.ctypes.data))

    bad_requests = ((_abi.BucketRequestC(0, 100, 4, lo, hi, 1, 1), b"which_mask"),
                    (_abi.BucketRequestC(0, 0, 4, lo, hi, 1, 0), b"width"),
                    (_abi.BucketRequestC(0, -5, 4, lo, hi, 1, 0), b"width"),
                    (_abi.BucketRequestC(0, 100, 4, lo, hi, 0, 0), b"n_groups must"),
                    (_abi.BucketRequestC(0, 100, (1 << 64) // 8, lo, hi, 4_000_000_000, 0), b"overflows"),
                    (_abi.BucketRequestC(0, 100, (1 << 60), lo, hi, 1, 0), b"overflows"))
    cases = []
    for request, message in bad_requests:
        cases += [(call, message) for call in hist_calls(request, edges, 2) + quantile_calls(request, q, 1)]
    for bad_edges, n_edges, message in ((edges, 0, b"n_edges"), (edges, mdb.MDB_HIST_MAX_EDGES + 1, b"n_edges"),
                                        (np.array([2.0, 1.0], dtype=np.float32), 2, b"strictly increasing"),
                                        (np.array([1.0, 1.0], dtype=np.float32), 2, b"strictly increasing"),
                                        (np.array([0.0, -0.0], dtype=np.float32), 2, b"strictly increasing"),
                                        (None, 2, b"NULL")):
        cases += [(call, message) for call in hist_calls(good, bad_edges, n_edges)]
    for bad_q, n_q, message in ((np.array([1.5]), 1, b"[0, 1]"), (np.array([-0.1]), 1, b"[0, 1]"),
                                (np.array([float("nan")]), 1, b"[0, 1]"), (q, 0, b"n_q"),
                                (np.full(5, 0.5), 5, b"n_q")):
        cases += [(call, message) for call in quantile_calls(good, bad_q, n_q)]
    for call, message in cases:
        assert call() == 1
        assert message in library.mdb_last_error(), (message, library.mdb_last_error())
        assert [a.tobytes() for a in (counts, lo_out, hi_out, n_points)] == before
    assert library.mdb_hist_buckets(None, None, None, None, None, 0, None) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_quantile_buckets(None, None, None, None, None, 0, None, None, None) == 1
    assert b"NULL" in library.mdb_last_error()


@pytest.fixture(scope="module")
def built():
    done = subprocess.run(["make", "-C", HERE, "all"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


@pytest.mark.parametrize("flavour", ["plain", "asan"])
def test_selection_step_without_a_gpu(built, flavour):
    """Every order statistic of every cell of random (cell, key) samples - NaNs, signed zeros, empty and one-point cells -
    equals the sorted cell's, by the passes and the step the device runs; the program alone carries the sanitizers."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    done = subprocess.run([os.path.join(HERE, "_build", f"check_{flavour}")], capture_output=True, text=True, env=env,
                          timeout=300)
    output = done.stdout + done.stderr
    assert done.returncode == 0, output[-4000:]
    assert output.startswith("ok: ") or "\nok: " in output, output[-4000:]
    for report in ("ERROR: AddressSanitizer", "runtime error:", "MISMATCH"):
        assert report not in output, output[-4000:]
