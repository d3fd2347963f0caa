"""CPU-side checks of the transitions operator (mdb_transit_buckets*): the entry points in the built library, the
header, the ctypes mirror and the Rust binding; the request and edge checks, made before the device is used; merge and
crossings on hand-made matrices; the reference of the GPU tests (tests/transit_cases.py) against hand-computed tables;
and the host side (modelardb-rs_amd/csrc/mdb_transit_host.cpp, the plain-C++ part of mdb_transit.hpp) driven by a
stand-alone program, plain and under AddressSanitizer + UBSan (tests/transit_host)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import modelardb_rs_amd as mdb
import transit_cases as tc
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "transit_host")
NAMES = ("mdb_transit_buckets", "mdb_transit_buckets_dev", "mdb_transit_buckets_list", "mdb_transit_merge_n",
         "mdb_transit_crossings")
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
    assert {name for name in declared | listed if "transit" in name} == set(NAMES)
    # the names stay out of the neighbours' pinned name sets
    for name in NAMES:
        assert not name.startswith("mdb_sample")
        for word in ("dwell", "change", "integral", "trend", "binned", "episodes", "comoments"):
            assert word not in name
    for method in ("transit_buckets", "transit_buckets_list", "transit_merge", "transit_crossings"):
        assert re.search(rf"pub fn {method}\(", wrappers), method
    for method in ("transit_buckets", "transit_buckets_list", "transit_buckets_dev", "transit"):
        assert callable(getattr(mdb.Context, method)), method
    assert callable(mdb.transit_merge) and callable(mdb.transit_crossings)


def test_entry_points_request_layout():
    layout = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    assert "typedef struct mdb_transit_request" in layout and "pub struct mdb_transit_request" in rust
    request = _abi.TransitRequestC
    assert ctypes.sizeof(request) == ctypes.sizeof(_abi.ChangeRequestC) == 64
    assert (request.buckets.offset, request.max_gap.offset, request.reserved.offset, request.flags.offset) == (0, 48, 56, 60)
    for member, offset in (("buckets", 0), ("max_gap", 48), ("reserved", 56), ("flags", 60)):
        assert f"offsetof(mdb_transit_request, {member}) == {offset})" in layout
        assert f"offset_of!(mdb_transit_request, {member}) == {offset})" in rust
    assert "sizeof(mdb_transit_request) == 64" in layout and "size_of::<mdb_transit_request>() == 64" in rust


def _request(origin=0, width=100, n_buckets=4, t_lo=I64_MIN, t_hi=I64_MAX, n_groups=1, which_mask=0, max_gap=I64_MAX,
             reserved=0, flags=0):
    request = _abi.TransitRequestC()
    request.buckets = _abi.BucketRequestC(origin, width, n_buckets, t_lo, t_hi, n_groups, which_mask)
    request.max_gap, request.reserved, request.flags = max_gap, reserved, flags
    return request


def test_requests_and_edges_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    counts = np.frombuffer(bytes([0xA5]) * (8 * 4 * 3 * 3), dtype=np.uint64).copy()
    before = counts.copy()
    pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
    groups = (ctypes.c_void_p * 1)(None)
    good_edges = np.array([0.0, 1.0], dtype=np.float32)

    def calls(request, edges, n_edges):
        e = None if edges is None else edges.ctypes.data
        return (lambda: library.mdb_transit_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(request), e,
                                                    n_edges, counts.ctypes.data),
                lambda: library.mdb_transit_buckets_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(request), e,
                                                        n_edges, counts.ctypes.data),
                lambda: library.mdb_transit_buckets_list(fake_context, pointers, groups, 1, ctypes.byref(request), e,
                                                         n_edges, counts.ctypes.data))

    for request, message in ((_request(which_mask=1), b"which_mask must be 0 for mdb_transit_buckets"),
                             (_request(width=0), b"width"),
                             (_request(width=-3), b"width"),
                             (_request(n_groups=0), b"n_groups must"),
                             (_request(n_buckets=(1 << 64) // 8, n_groups=4_000_000_000), b"overflows"),
                             (_request(n_buckets=(1 << 60) // 9 + 1, n_groups=1), b"overflows"),
                             (_request(t_lo=0), b"time range"),
                             (_request(t_hi=I64_MAX - 1), b"time range"),
                             (_request(reserved=1), b"reserved"),
                             (_request(flags=1), b"flags"),
                             (_request(max_gap=-1), b"max_gap"),
                             (_request(max_gap=I64_MIN), b"max_gap")):
        for call in calls(request, good_edges, 2):
            assert call() == 1
            assert message in library.mdb_last_error(), (message, library.mdb_last_error())
        assert counts.tobytes() == before.tobytes()
    # the counters grow with the SQUARE of the cells: 2^36 rows overflow under 4 095 edges
    many_edges = np.arange(mdb.MDB_HIST_MAX_EDGES, dtype=np.float32)
    for call in calls(_request(n_buckets=1 << 36), many_edges, mdb.MDB_HIST_MAX_EDGES):
        assert call() == 1 and b"overflows" in library.mdb_last_error()
    request = _request()
    for edges, n_edges, message in ((np.array([1.0, 0.0], dtype=np.float32), 2, b"strictly increasing"),
                                    (np.array([1.0, 1.0], dtype=np.float32), 2, b"strictly increasing"),
                                    (np.array([0.0, -0.0], dtype=np.float32), 2, b"strictly increasing"),
                                    (np.array([np.nan, 1.0], dtype=np.float32), 2, b"strictly increasing"),
                                    (good_edges, 0, b"n_edges"),
                                    (good_edges, mdb.MDB_HIST_MAX_EDGES + 1, b"n_edges"),
                                    (None, 2, b"NULL")):
        for call in calls(request, edges, n_edges):
            assert call() == 1
            assert message in library.mdb_last_error(), (message, library.mdb_last_error())
        assert counts.tobytes() == before.tobytes()
    e = good_edges.ctypes.data
    assert library.mdb_transit_buckets(None, None, None, None, None, 0, None) == 1 and b"NULL" in library.mdb_last_error()
    for arguments in ((None, ctypes.byref(seg), None, ctypes.byref(request), e, 2, counts.ctypes.data),
                      (fake_context, None, None, ctypes.byref(request), e, 2, counts.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, None, e, 2, counts.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, ctypes.byref(request), e, 2, None)):
        assert library.mdb_transit_buckets(*arguments) == 1 and b"NULL" in library.mdb_last_error()
        assert library.mdb_transit_buckets_dev(*arguments) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_transit_buckets_list(fake_context, None, None, 1, ctypes.byref(request), e, 2, counts.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    missing = (ctypes.POINTER(_abi.SegmentsC) * 1)()
    assert library.mdb_transit_buckets_list(fake_context, missing, groups, 1, ctypes.byref(request), e, 2,
                                            counts.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    # nothing to do: success without a context that could be used
    no_buckets = _request(n_buckets=0)
    assert library.mdb_transit_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(no_buckets), e, 2,
                                       counts.ctypes.data) == 0
    assert library.mdb_transit_buckets_list(fake_context, pointers, groups, 0, ctypes.byref(request), e, 2,
                                            counts.ctypes.data) == 0
    assert counts.tobytes() == before.tobytes()


def test_merge_and_crossings_on_the_host():
    # one (group, bucket) row under two edges: [from][to]
    counts = np.array([[[[1, 2, 3], [4, 5, 6], [7, 8, 9]], [[0, 0, 1], [0, 0, 0], [0, 0, 0]]]], dtype=np.uint64)
    up, down = mdb.transit_crossings(counts)
    assert up.shape == down.shape == (1, 2, 2) and up.dtype == down.dtype == np.uint64
    # edge 0: up 0 -> 1 and 0 -> 2, down 1 -> 0 and 2 -> 0; edge 1: up 0 -> 2 and 1 -> 2, down 2 -> 0 and 2 -> 1
    assert up[0, 0].tolist() == [2 + 3, 3 + 6] and down[0, 0].tolist() == [4 + 7, 7 + 8]
    assert up[0, 1].tolist() == [1, 1] and down[0, 1].tolist() == [0, 0]   # a jump over two edges crosses both
    reference_up, reference_down = tc.crossings(counts)
    np.testing.assert_array_equal(up, reference_up)
    np.testing.assert_array_equal(down, reference_down)
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 1000, size=(3, 2, 17, 17)).astype(np.uint64)
    up, down = mdb.transit_crossings(wide)
    reference_up, reference_down = tc.crossings(wide)
    np.testing.assert_array_equal(up, reference_up)
    np.testing.assert_array_equal(down, reference_down)
    np.testing.assert_array_equal(up[..., 0], wide[..., 0, 1:].sum(axis=-1))
    one_cell = mdb.transit_crossings(np.array([[7]], dtype=np.uint64))
    assert one_cell[0].shape == one_cell[1].shape == (0,)
    for wrong in (np.zeros(3), np.zeros((2, 3), dtype=np.uint64), np.zeros(4, dtype=np.uint64)):
        with pytest.raises(ValueError):
            mdb.transit_crossings(wrong)
    other = np.arange(18, dtype=np.uint64).reshape(counts.shape)
    merged = mdb.transit_merge(counts.copy(), other)
    np.testing.assert_array_equal(merged, counts + other)
    top = np.array([(1 << 64) - 1, 5], dtype=np.uint64)
    assert mdb.transit_merge(top, np.array([2, 1], dtype=np.uint64)).tolist() == [1, 6]   # (the integers wrap)
    with pytest.raises(ValueError):
        mdb.transit_merge(counts, other[:, :1])
    with pytest.raises(ValueError):
        mdb.transit_merge(counts, np.zeros(counts.shape))


def test_the_reference_against_hand_computed_tables():
    f = np.float32
    # rows (t, v): 0:1, 100:3, 200:3, 300:2.5, 300:9 (time stands still), 450:0.5, 2000:8 (a long gap), 2100:nan, 2200:1
    timestamps = [0, 100, 200, 300, 300, 450, 2000, 2100, 2200]
    values = np.array([1, 3, 3, 2.5, 9, 0.5, 8, np.nan, 1], dtype=np.float32)
    edges = np.array([1.0, 3.0], dtype=np.float32)   # cells: below 1 | [1, 3) | 3 and above (a value ON an edge lies above it)
    got = tc.rows_oracle(timestamps, values, edges, 3, 50, 1000, max_gap=1000)
    # bucket 0 is [50, 1050): 1 -> 3 (its earlier row lies in front of the origin), 3 -> 3, 3 -> 2.5, 9 -> 0.5; 300 -> 300
    # is not linked; 450 -> 2000 is cut by the gap. Bucket 1 is [1050, 2050): nothing. Bucket 2: 8 -> NaN and NaN -> 1
    assert got.shape == (1, 3, 3, 3) and got.dtype == np.uint64
    assert got[0, 0].tolist() == [[0, 0, 0], [0, 0, 1], [1, 1, 1]]
    assert got[0, 1].tolist() == [[0, 0, 0]] * 3
    assert got[0, 2].tolist() == [[0, 0, 0], [0, 0, 0], [0, 1, 1]]
    # no gap rule: 0.5 -> 8 arrives in bucket 1, the bucket of its LATER row
    free = tc.rows_oracle(timestamps, values, edges, 3, 50, 1000)
    assert free[0, 1].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0]] and int(free.sum()) == int(got.sum()) + 1
    up, down = tc.crossings(free)
    assert up[0].tolist() == [[0, 1], [1, 1], [0, 0]] and down[0].tolist() == [[1, 2], [0, 0], [0, 1]]
    # the sign of a NaN and of a zero place them
    special = np.array([0, -0.0, 0.0, -np.inf, np.inf, 7.0], dtype=np.float32)
    special[0] = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    zero_edge = np.array([0.0], dtype=np.float32)
    got = tc.rows_oracle([0, 10, 30, 60, 100, 150], special, zero_edge, 1, 0, 1000)
    # -NaN -> -0.0 stays below; -0.0 -> +0.0 goes up; +0.0 -> -inf down; -inf -> +inf up; +inf -> 7 stays above
    assert got[0, 0].tolist() == [[1, 2], [1, 1]]
    # groups: a change of group links nothing; a pair whose later row lies behind the last bucket is dropped
    got = tc.rows_oracle([0, 100, 200, 300], [f(1), f(1), f(5), f(5)], edges, 2, 50, 100, row_groups=[0, 0, 1, 1], n_groups=2)
    assert got[0, 0, 1, 1] == 1 and got[1].sum() == 0 and got.sum() == 1   # (300 lies behind [50, 250))
    # a pair is never cut: one link over three buckets counts once, in the last
    got = tc.rows_oracle([130, 370], [f(2), f(0)], edges, 5, 0, 100)
    assert got[0, 3, 1, 0] == 1 and int(got.sum()) == 1
    # Python integers: nothing wraps at the int64 extremes (bucket 1 starts at -1, bucket 2 at INT64_MAX - 1)
    got = tc.rows_oracle([I64_MIN, -1, I64_MAX], [f(0), f(2), f(2)], edges, 3, I64_MIN, I64_MAX)
    assert got[0, 1, 0, 1] == 1 and got[0, 2, 1, 1] == 1 and int(got.sum()) == 2


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
