"""CPU-side checks of the change operator (mdb_change_buckets*): the entry points in the built library, the header, the
ctypes mirror and the Rust binding; the request checks, made before the device is used; merge and finish on hand-made
cells; the reference of the GPU tests (tests/change_cases.py) against hand-computed cells; and the host side
(modelardb-rs_amd/csrc/mdb_change_host.cpp, the plain-C++ part of mdb_change.hpp) driven by a stand-alone program,
plain and under AddressSanitizer + UBSan (tests/change_host)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import change_cases as chc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "change_host")
NAMES = ("mdb_change_buckets", "mdb_change_buckets_dev", "mdb_change_buckets_list", "mdb_change_merge_n",
         "mdb_change_finish")
MEMBERS = ("count", "n_fall", "duration", "rise", "fall", "reset_sum", "max_rise", "max_fall")
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
    assert {name for name in declared | listed if "change" in name} == set(NAMES)
    for method in ("change_buckets", "change_buckets_list", "change_merge", "change_finish"):
        assert re.search(rf"pub fn {method}\(", wrappers), method
    for method in ("change_buckets", "change_buckets_list", "change_buckets_dev", "change"):
        assert callable(getattr(mdb.Context, method)), method
    assert callable(mdb.change_merge) and callable(mdb.change_finish) and callable(mdb.fresh_change_cells)
    # the layouts: the header's, the ctypes mirror's, numpy's and the Rust binding's
    assert "typedef struct mdb_change_cell" in layout and "typedef struct mdb_change_request" in layout
    kinds = (("NET", 0), ("VARIATION", 1), ("INCREASE", 2), ("RATE", 3))
    for kind, number in kinds:
        assert re.search(rf"#define MDB_CHANGE_{kind}\s+{number}u", layout), kind
        assert f"pub const MDB_CHANGE_{kind}: u32 = {number};" in rust, kind
        assert getattr(mdb, f"MDB_CHANGE_{kind}") == number
    cell = mdb.CHANGE_CELL_DTYPE
    assert cell == chc.CELL_DTYPE and ctypes.sizeof(_abi.ChangeCellC) == cell.itemsize == 64
    assert cell.names == MEMBERS
    assert f"sizeof(mdb_change_cell) == 64" in layout and "size_of::<mdb_change_cell>() == 64" in rust
    for k, member in enumerate(MEMBERS):
        assert cell.fields[member][1] == 8 * k and getattr(_abi.ChangeCellC, member).offset == 8 * k
        assert f"offsetof(mdb_change_cell, {member}) == {8 * k})" in layout, member
        assert f"offset_of!(mdb_change_cell, {member}) == {8 * k})" in rust, member
    request = _abi.ChangeRequestC
    assert ctypes.sizeof(request) == 64
    assert (request.buckets.offset, request.max_gap.offset, request.reserved.offset, request.flags.offset) == (0, 48, 56, 60)
    for member, offset in (("max_gap", 48), ("reserved", 56), ("flags", 60)):
        assert f"offsetof(mdb_change_request, {member}) == {offset})" in layout
        assert f"offset_of!(mdb_change_request, {member}) == {offset})" in rust
    assert "sizeof(mdb_change_request) == 64" in layout and "size_of::<mdb_change_request>() == 64" in rust


def _request(origin=0, width=100, n_buckets=4, t_lo=I64_MIN, t_hi=I64_MAX, n_groups=1, which_mask=0, max_gap=I64_MAX,
             reserved=0, flags=0):
    request = _abi.ChangeRequestC()
    request.buckets = _abi.BucketRequestC(origin, width, n_buckets, t_lo, t_hi, n_groups, which_mask)
    request.max_gap, request.reserved, request.flags = max_gap, reserved, flags
    return request


def test_requests_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    cells = np.frombuffer(bytes([0xA5]) * (64 * 4), dtype=mdb.CHANGE_CELL_DTYPE).copy()
    before = cells.copy()
    pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
    groups = (ctypes.c_void_p * 1)(None)
    for request, message in ((_request(which_mask=1), b"which_mask must be 0 for mdb_change_buckets"),
                             (_request(width=0), b"width"),
                             (_request(width=-3), b"width"),
                             (_request(n_groups=0), b"n_groups must"),
                             (_request(n_buckets=(1 << 64) // 8, n_groups=4_000_000_000), b"overflows"),
                             (_request(n_buckets=(1 << 64) // 64, n_groups=1), b"overflows"),
                             (_request(t_lo=0), b"time range"),
                             (_request(t_hi=I64_MAX - 1), b"time range"),
                             (_request(reserved=1), b"reserved"),
                             (_request(flags=1), b"flags"),
                             (_request(max_gap=-1), b"max_gap"),
                             (_request(max_gap=I64_MIN), b"max_gap")):
        for call in (lambda: library.mdb_change_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(request),
                                                        cells.ctypes.data),
                     lambda: library.mdb_change_buckets_dev(fake_context, ctypes.byref(seg), None,
                                                            ctypes.byref(request), cells.ctypes.data),
                     lambda: library.mdb_change_buckets_list(fake_context, pointers, groups, 1, ctypes.byref(request),
                                                             cells.ctypes.data)):
            assert call() == 1
            assert message in library.mdb_last_error(), (message, library.mdb_last_error())
        assert cells.tobytes() == before.tobytes()
    request = _request()
    assert library.mdb_change_buckets(None, None, None, None, None) == 1 and b"NULL" in library.mdb_last_error()
    for arguments in ((None, ctypes.byref(seg), None, ctypes.byref(request), cells.ctypes.data),
                      (fake_context, None, None, ctypes.byref(request), cells.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, None, cells.ctypes.data),
                      (fake_context, ctypes.byref(seg), None, ctypes.byref(request), None)):
        assert library.mdb_change_buckets(*arguments) == 1 and b"NULL" in library.mdb_last_error()
        assert library.mdb_change_buckets_dev(*arguments) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_change_buckets_list(fake_context, None, None, 1, ctypes.byref(request), cells.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    missing = (ctypes.POINTER(_abi.SegmentsC) * 1)()
    assert library.mdb_change_buckets_list(fake_context, missing, groups, 1, ctypes.byref(request), cells.ctypes.data) == 1
    assert b"NULL" in library.mdb_last_error()
    # nothing to do: success without a context that could be used
    no_buckets = _request(n_buckets=0)
    assert library.mdb_change_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(no_buckets), cells.ctypes.data) == 0
    assert library.mdb_change_buckets_list(fake_context, pointers, groups, 0, ctypes.byref(request), cells.ctypes.data) == 0
    assert cells.tobytes() == before.tobytes()


def _cells(rows):
    cells = mdb.fresh_change_cells(len(rows))
    for k, row in enumerate(rows):
        cells[k] = row
    return cells


def test_merge_and_finish_on_the_host():
    assert mdb.fresh_change_cells((2, 3)).tobytes() == bytes(6 * 64)
    nan, inf = np.nan, np.inf
    cells = _cells([(0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0),            # nothing
                    (4, 1, 2_000_000, 10.0, 4.0, 1.0, 6.0, 4.0),    # two seconds
                    (2, 0, 0, 3.0, 0.0, 0.0, 3.0, 0.0),             # duration 0 (merged by hand: never from a call)
                    (2, 0, 10, nan, nan, 0.0, 0.0, 0.0),            # poisoned
                    (1, 1, 500_000, 0.0, inf, -inf, 0.0, inf)])     # a fall to -inf
    net = mdb.change_finish(cells, mdb.MDB_CHANGE_NET)
    assert np.isnan(net[0]) and net[1] == 6.0 and net[2] == 3.0 and np.isnan(net[3]) and net[4] == -inf
    variation = mdb.change_finish(cells, mdb.MDB_CHANGE_VARIATION)
    assert np.isnan(variation[0]) and variation[1] == 14.0 and variation[2] == 3.0 and np.isnan(variation[3]) and variation[4] == inf
    increase = mdb.change_finish(cells, mdb.MDB_CHANGE_INCREASE)
    assert np.isnan(increase[0]) and increase[1] == 11.0 and increase[2] == 3.0 and np.isnan(increase[3]) and increase[4] == -inf
    rate = mdb.change_finish(cells, mdb.MDB_CHANGE_RATE)
    assert np.isnan(rate[0]) and rate[1] == 5.5 and np.isnan(rate[2]) and np.isnan(rate[3]) and rate[4] == -inf
    assert mdb.change_finish(cells[:4].reshape(2, 2), mdb.MDB_CHANGE_NET).shape == (2, 2)
    with pytest.raises(mdb.HipError, match="kind"):
        mdb.change_finish(cells, 4)
    with pytest.raises(ValueError):
        mdb.change_finish(np.zeros(3), mdb.MDB_CHANGE_NET)
    other = _cells([(1, 0, 7, 1.5, 0.0, 0.0, 1.5, 0.0),
                    (2, 1, 20, 0.5, 3.0, 1.0, 0.5, 7.0),
                    ((1 << 64) - 2, (1 << 64) - 1, (1 << 64) - 1, 1.0, 0.0, 0.0, 9.0, 0.0),
                    (1, 0, 5, 1.0, 1.0, 2.0, 4.0, 0.0),
                    (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)])
    merged = mdb.change_merge(cells.copy(), other)
    assert merged[0].tobytes() == other[0].tobytes()          # a fresh cell takes the other whole
    assert merged[1].tolist() == (6, 2, 2_000_020, 10.5, 7.0, 2.0, 6.0, 7.0)
    assert merged[2].tolist() == (0, (1 << 64) - 1, (1 << 64) - 1, 4.0, 0.0, 0.0, 9.0, 0.0)   # (the integers wrap)
    assert merged["count"][3] == 3 and merged["duration"][3] == 15 and np.isnan(merged["rise"][3]) and np.isnan(merged["fall"][3])
    assert merged["reset_sum"][3] == 2.0 and merged["max_rise"][3] == 4.0 and merged["max_fall"][3] == 0.0
    assert merged[4].tobytes() == cells[4].tobytes()          # merging a fresh cell changes nothing
    with pytest.raises(ValueError):
        mdb.change_merge(cells, other[:3])
    with pytest.raises(ValueError):
        mdb.change_merge(cells, np.zeros(5))


def test_the_reference_against_hand_computed_cells():
    f = np.float32
    # rows (t, v): 0:1, 100:3, 200:3, 300:2.5, 300:9 (time stands still), 450:0.5, 2000:8 (a long gap), 2100:nan, 2200:1
    timestamps = [0, 100, 200, 300, 300, 450, 2000, 2100, 2200]
    values = [f(1), f(3), f(3), f(2.5), f(9), f(0.5), f(8), f(np.nan), f(1)]
    got = chc.rows_oracle(timestamps, values, 3, 50, 1000, max_gap=1000)
    # bucket 0 is [50, 1050): pairs ending at 100 (+2), 200 (0), 300 (-0.5), 450 (-8.5); 300 -> 300 is not linked
    assert got["count"].tolist() == [[4, 0, 2]] and got["n_fall"].tolist() == [[2, 0, 0]]
    assert got["duration"].tolist() == [[100 + 100 + 100 + 150, 0, 200]]
    assert got["rise"].tolist() == [[2.0, 0.0, 0.0]] and got["fall"].tolist() == [[9.0, 0.0, 0.0]]
    assert got["reset_sum"].tolist() == [[3.0, 0.0, 0.0]]
    assert got["max_rise"].tolist() == [[2.0, 0.0, 0.0]] and got["max_fall"].tolist() == [[8.5, 0.0, 0.0]]
    assert got["poisoned"].tolist() == [[False, False, True]]   # 2000 -> 2100 -> 2200 read the NaN; 450 -> 2000 is cut by the gap
    assert got["scale_rise"].tolist() == [[2.0, 0.0, 0.0]] and got["scale_reset_sum"].tolist() == [[3.0, 0.0, 0.0]]
    # no gap rule: the pair ending at 2000 (+7.5) lands in bucket 1 and spans 1550 microseconds
    free = chc.rows_oracle(timestamps, values, 3, 50, 1000)
    assert free["count"].tolist() == [[4, 1, 2]] and free["duration"].tolist() == [[450, 1550, 200]]
    assert free["rise"][0, 1] == 7.5 and free["max_rise"][0, 1] == 7.5
    # d is the f64 difference of the two f32 values: one rounding
    tenth = chc.rows_oracle([0, 10], [f(0.1), f(0.3)], 1, 0, 100)
    assert tenth["rise"][0, 0] == np.float64(f(0.3)) - np.float64(f(0.1)) != 0.2
    # a later row outside the buckets drops the pair; an earlier row before the origin does not
    outside = chc.rows_oracle([0, 100, 300], [f(1), f(2), f(4)], 2, 50, 100)
    assert outside["count"].tolist() == [[1, 0]] and outside["rise"][0, 0] == 1.0
    # assert_cells: accepts the reference's own cells, sees a wrong integer, a sum beyond the tolerance and a missing NaN
    cells = np.zeros((1, 3), dtype=chc.CELL_DTYPE)
    for name in chc.EXACT + chc.SUMS:
        cells[name] = got[name]
    cells["rise"][0, 2] = cells["fall"][0, 2] = np.nan
    assert chc.assert_cells(cells, got, "hand") == (1, 1)
    for name, cell, value in (("n_fall", 0, 1), ("rise", 0, 2.0 + 2.0 ** -48), ("max_fall", 0, 8.5000001), ("rise", 2, 0.0),
                              ("count", 1, 1)):
        wrong = cells.copy()
        wrong[name][0, cell] = value
        with pytest.raises(AssertionError):
            chc.assert_cells(wrong, got, "hand, wrong")
    near = cells.copy()
    near["rise"][0, 0] = 2.0 + 2.0 ** -51   # (4 pairs x 2^-52 x S = 2: 2^-49 allowed)
    chc.assert_cells(near, got, "hand, within tolerance")


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
