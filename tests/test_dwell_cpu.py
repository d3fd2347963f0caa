"""CPU-side checks of the dwell operator (mdb_dwell_buckets*): the entry points in the built library, the header, the
ctypes mirror and the Rust binding; the request and edge checks, made before the device is used; merge and share on
hand-made counters; the reference of the GPU tests (tests/dwell_cases.py) against hand-computed tables; and the host
side (modelardb-rs_amd/csrc/mdb_dwell_host.cpp, the plain-C++ part of mdb_dwell.hpp) driven by a stand-alone program,
plain and under AddressSanitizer + UBSan (tests/dwell_host)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dwell_cases as dc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "dwell_host")
NAMES = ("mdb_dwell_buckets", "mdb_dwell_buckets_dev", "mdb_dwell_buckets_list", "mdb_dwell_merge_n", "mdb_dwell_share")
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
    assert {name for name in declared | listed if "dwell" in name} == set(NAMES)
    for method in ("dwell_buckets", "dwell_buckets_list", "dwell_merge", "dwell_share"):
        assert re.search(rf"pub fn {method}\(", wrappers), method
    for method in ("dwell_buckets", "dwell_buckets_list", "dwell_buckets_dev", "dwell"):
        assert callable(getattr(mdb.Context, method)), method
    assert callable(mdb.dwell_merge) and callable(mdb.dwell_share)
    # the request: the header's layout, the ctypes mirror's and the Rust binding's; the method's number
    assert "typedef struct mdb_dwell_request" in layout
    assert re.search(r"#define MDB_DWELL_STEP\s+1u", layout) and "pub const MDB_DWELL_STEP: u32 = 1;" in rust
    assert mdb.MDB_DWELL_STEP == mdb.MDB_INTEGRAL_STEP == dc.STEP == 1
    request = _abi.DwellRequestC
    assert ctypes.sizeof(request) == ctypes.sizeof(_abi.IntegralRequestC) == 64
    assert (request.buckets.offset, request.max_gap.offset, request.method.offset, request.flags.offset) == (0, 48, 56, 60)
    for member, offset in (("buckets", 0), ("max_gap", 48), ("method", 56), ("flags", 60)):
        assert f"offsetof(mdb_dwell_request, {member}) == {offset})" in layout
        assert f"offset_of!(mdb_dwell_request, {member}) == {offset})" in rust
    assert "sizeof(mdb_dwell_request) == 64" in layout and "size_of::<mdb_dwell_request>() == 64" in rust
    # the header says why there is no linear method
    assert "MDB_INTEGRAL_LINEAR's number (0) is refused" in header


def _request(origin=0, width=100, n_buckets=4, t_lo=I64_MIN, t_hi=I64_MAX, n_groups=1, which_mask=0, max_gap=I64_MAX,
             method=1, flags=0):
    request = _abi.DwellRequestC()
    request.buckets = _abi.BucketRequestC(origin, width, n_buckets, t_lo, t_hi, n_groups, which_mask)
    request.max_gap, request.method, request.flags = max_gap, method, flags
    return request


def test_requests_and_edges_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    dwell = np.frombuffer(bytes([0xA5]) * (8 * 4 * 3), dtype=np.uint64).copy()
    before = dwell.copy()
    pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
    groups = (ctypes.c_void_p * 1)(None)
    good_edges = np.array([0.0, 1.0], dtype=np.float32)

    def calls(request, edges, n_edges):
        e = None if edges is None else edges.ctypes.data
        return (lambda: library.mdb_dwell_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(request), e, n_edges,
                                                  dwell.ctypes.data),
                lambda: library.mdb_dwell_buckets_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(request), e,
                                                      n_edges, dwell.ctypes.data),
                lambda: library.mdb_dwell_buckets_list(fake_context, pointers, groups, 1, ctypes.byref(request), e, n_edges,
                                                       dwell.ctypes.data))

    for request, message in ((_request(which_mask=1), b"which_mask must be 0 for mdb_dwell_buckets"),
                             (_request(width=0), b"width"),
                             (_request(width=-3), b"width"),
                             (_request(n_groups=0), b"n_groups must"),
                             (_request(n_buckets=(1 << 64) // 8, n_groups=4_000_000_000), b"overflows"),
                             (_request(n_buckets=(1 << 60) // 3 + 1, n_groups=1), b"overflows"),
                             (_request(t_lo=0), b"time range"),
                             (_request(t_hi=I64_MAX - 1), b"time range"),
                             (_request(method=0), b"MDB_INTEGRAL_LINEAR"),
                             (_request(method=2), b"Unknown method"),
                             (_request(flags=1), b"flags"),
                             (_request(max_gap=-1), b"max_gap"),
                             (_request(max_gap=I64_MIN), b"max_gap")):
        for call in calls(request, good_edges, 2):
            assert call() == 1
            assert message in library.mdb_last_error(), (message, library.mdb_last_error())
        assert dwell.tobytes() == before.tobytes()
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
        assert dwell.tobytes() == before.tobytes()
    e = good_edges.ctypes.data
    assert library.mdb_dwell_buckets(None, None, None, None, None, 0, None) == 1 and b"NULL" in library.mdb_last_error()
    for arguments in ((None, ctypes.byref(seg), None, ctypes.byref(request), e, 2, dwell.ctypes.data),
                      (fake_context, None, None, ctypes.byref(request), e, 2, dwell.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, None, e, 2, dwell.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, ctypes.byref(request), e, 2, None)):
        assert library.mdb_dwell_buckets(*arguments) == 1 and b"NULL" in library.mdb_last_error()
        assert library.mdb_dwell_buckets_dev(*arguments) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_dwell_buckets_list(fake_context, None, None, 1, ctypes.byref(request), e, 2, dwell.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    missing = (ctypes.POINTER(_abi.SegmentsC) * 1)()
    assert library.mdb_dwell_buckets_list(fake_context, missing, groups, 1, ctypes.byref(request), e, 2,
                                          dwell.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    # nothing to do: success without a context that could be used
    no_buckets = _request(n_buckets=0)
    assert library.mdb_dwell_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(no_buckets), e, 2, dwell.ctypes.data) == 0
    assert library.mdb_dwell_buckets_list(fake_context, pointers, groups, 0, ctypes.byref(request), e, 2, dwell.ctypes.data) == 0
    assert dwell.tobytes() == before.tobytes()


def test_merge_and_share_on_the_host():
    dwell = np.array([[[1, 1, 2], [0, 0, 0]], [[5, 0, 0], [(1 << 64) - 1, (1 << 64) - 1, 0]]], dtype=np.uint64)
    share = mdb.dwell_share(dwell)
    assert share.shape == dwell.shape and share.dtype == np.float64
    assert share[0, 0].tolist() == [0.25, 0.25, 0.5] and np.isnan(share[0, 1]).all()
    assert share[1, 0].tolist() == [1.0, 0.0, 0.0] and share[1, 1].tolist() == [0.5, 0.5, 0.0]
    assert mdb.dwell_share(np.array([3, 1], dtype=np.uint64)).tolist() == [0.75, 0.25]
    assert mdb.dwell_share(np.zeros((2, 0), dtype=np.uint64)).shape == (2, 0)
    with pytest.raises(ValueError):
        mdb.dwell_share(np.zeros(3))
    other = np.array([[[1, 2, 3], [4, 5, 6]], [[7, 8, 9], [1, 2, 3]]], dtype=np.uint64)
    merged = mdb.dwell_merge(dwell.copy(), other)
    assert merged[0].tolist() == [[2, 3, 5], [4, 5, 6]] and merged[1, 0].tolist() == [12, 8, 9]
    assert merged[1, 1].tolist() == [0, 1, 3]           # (the integers wrap)
    with pytest.raises(ValueError):
        mdb.dwell_merge(dwell, other[:1])
    with pytest.raises(ValueError):
        mdb.dwell_merge(dwell, np.zeros(dwell.shape))


def test_the_reference_against_hand_computed_tables():
    f = np.float32
    # rows (t, v): 0:1, 100:3, 200:3, 300:2.5, 300:9 (time stands still), 450:0.5, 2000:8 (a long gap), 2100:nan, 2200:1
    timestamps = [0, 100, 200, 300, 300, 450, 2000, 2100, 2200]
    values = np.array([1, 3, 3, 2.5, 9, 0.5, 8, np.nan, 1], dtype=np.float32)
    edges = np.array([1.0, 3.0], dtype=np.float32)   # cells: below 1 | [1, 3) | 3 and above (a value ON an edge lies above it)
    got = dc.rows_oracle(timestamps, values, edges, 3, 50, 1000, max_gap=1000)
    # bucket 0 is [50, 1050): 1 held on [50, 100), 3 on [100, 300), 2.5 nowhere (300 -> 300 is not linked), 9 on
    # [300, 450); 450 -> 2000 is cut by the gap. 8 is held on [2000, 2100), cut at 2050 between buckets 1 and 2; NaN on
    # [2100, 2200) lies in the last cell
    assert got.shape == (1, 3, 3) and got.dtype == np.uint64
    assert got[0].tolist() == [[0, 50, 200 + 150], [0, 0, 50], [0, 0, 50 + 100]]
    # no gap rule: 0.5 is held on [450, 2000), cut at 1050
    free = dc.rows_oracle(timestamps, values, edges, 3, 50, 1000)
    assert free[0].tolist() == [[600, 50, 350], [950, 0, 50], [0, 0, 50 + 100]]
    # the sign of a NaN and of a zero place them; the last row holds nothing; v1 is never read
    special = np.array([-np.nan, -0.0, 0.0, -np.inf, np.inf, 7.0], dtype=np.float32)
    special[0] = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    zero_edge = np.array([0.0], dtype=np.float32)
    got = dc.rows_oracle([0, 10, 30, 60, 100, 150], special, zero_edge, 1, 0, 1000)
    assert got[0, 0].tolist() == [10 + 20 + 40, 30 + 50]   # -NaN, -0.0 and -inf below the edge at +0.0; +0.0 and +inf at or above
    # groups: a change of group links nothing; an interval before the origin is clipped, one behind the last bucket dropped
    got = dc.rows_oracle([0, 100, 200, 300], [f(1), f(1), f(5), f(5)], edges, 2, 50, 100, row_groups=[0, 0, 1, 1], n_groups=2)
    assert got.tolist() == [[[0, 50, 0], [0, 0, 0]], [[0, 0, 0], [0, 0, 50]]]
    # a link that crosses three buckets, its first and last partial; a bucket inside one link
    got = dc.rows_oracle([130, 370], [f(2), f(0)], edges, 5, 0, 100)
    assert got[0, :, 1].tolist() == [0, 70, 100, 70, 0] and int(got.sum()) == 240
    # Python integers: nothing wraps at the int64 extremes
    got = dc.rows_oracle([I64_MIN, -1, I64_MAX], [f(0), f(2), f(2)], edges, 3, I64_MIN, I64_MAX)
    assert got[0].tolist() == [[I64_MAX, 0, 0], [0, I64_MAX, 0], [0, 1, 0]]
    # edges_through: distinct, ascending, inside the data
    spread = dc.edges_through(np.array([100.0, 200.0], dtype=np.float32), 16)
    assert len(spread) == 16 and (np.diff(spread) > 0).all() and 100.0 < spread[0] and spread[-1] < 200.0


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
