"""CPU-side checks of the value histograms and quantiles (mdb_hist_*, mdb_quantile_*): the cell rule and the ranks of a
quantile through the C ABI against numpy on totalOrder keys, the edge lists they reject, the layout of
mdb_hist_request in the header, the ctypes mirror and the Rust binding, the entry points in the built library, and the
host arithmetic behind the quantile refinement (modelardb-rs_amd/csrc/mdb_hist.hpp) driven by a stand-alone program,
plain and under AddressSanitizer + UBSan (tests/hist_host)."""

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
HERE = os.path.join(REPO_ROOT, "tests", "hist_host")
NAMES = ("mdb_hist_batch", "mdb_hist_batch_dev", "mdb_hist_batch_list", "mdb_quantile_batch", "mdb_quantile_batch_dev",
         "mdb_hist_cell_of", "mdb_quantile_positions")


def _keys(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _special_values():
    """Finite values and their nextafter neighbours, ±0.0, ±inf, ±NaN (several payloads), subnormals, the extremes."""
    finite = np.array([1.0, -1.0, 37.0, 0.1, -0.1, 1e-40, -1e-40, 3.4028235e38, -3.4028235e38, 1.1754942e-38, 16777216.0,
                       100.0, 100.5], dtype=np.float32)
    with np.errstate(over="ignore"):  # (the neighbours of ±f32::MAX are the infinities)
        near = np.concatenate([np.nextafter(finite, np.float32(-np.inf)), finite, np.nextafter(finite, np.float32(np.inf))])
    special = _f32([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,
                    0x7FFFFFFF, 0xFFFFFFFF, 0x00000001, 0x80000001])
    return np.concatenate([near, special])


def test_cell_rule_equals_searchsorted_on_keys():
    values = _special_values()
    order = np.argsort(_keys(values), kind="stable")
    distinct = values[order][np.concatenate([[True], np.diff(_keys(values)[order]) > 0])]
    rng = np.random.default_rng(12)
    edge_lists = [distinct, distinct[::2], distinct[1::3], distinct[:1], distinct[-1:], _f32([0x80000000, 0x00000000]),
                  _f32([0x80000000, 0x00000000, 0x7F800000, 0x7FC00000])]
    edge_lists += [np.sort(rng.choice(len(distinct), size=5, replace=False)) for _ in range(4)]
    for edges in edge_lists:
        if edges.dtype != np.float32:
            edges = distinct[edges]
        expected = np.searchsorted(_keys(edges), _keys(values), side="right")
        got = [mdb.hist_cell_of(edges, v) for v in values]
        assert got == expected.tolist(), edges.view(np.uint32)
    # -0.0 lies below an edge at +0.0, +0.0 at it; a NaN lands where its key puts it
    assert mdb.hist_cell_of(_f32([0x00000000]), _f32([0x80000000])[0]) == 0
    assert mdb.hist_cell_of(_f32([0x00000000]), np.float32(0.0)) == 1
    assert mdb.hist_cell_of(np.array([np.inf], dtype=np.float32), np.float32(np.nan)) == 1
    assert mdb.hist_cell_of(np.array([-np.inf], dtype=np.float32), _f32([0xFFC00000])[0]) == 0


def test_bad_edge_lists_are_rejected():
    one = np.float32(1.0)
    bad = {"equal": [one, one], "descending": [np.float32(2.0), one], "-0.0 after +0.0": _f32([0x00000000, 0x80000000]),
           "none": np.zeros(0, dtype=np.float32), "4096 edges": np.arange(4096, dtype=np.float32),
           "equal NaNs": _f32([0x7FC00000, 0x7FC00000])}
    for name, edges in bad.items():
        with pytest.raises(mdb.HipError):
            mdb.hist_cell_of(edges, 0.0)
    assert mdb.hist_cell_of(np.arange(4095, dtype=np.float32), 5000.0) == 4095
    library = mdb.load_hip_library()
    cell = ctypes.c_uint32(77)
    assert library.mdb_hist_cell_of(None, 1, 0.0, ctypes.byref(cell)) == 1 and cell.value == 77
    assert b"NULL" in library.mdb_last_error()
    edges = np.array([1.0], dtype=np.float32)
    assert library.mdb_hist_cell_of(edges.ctypes.data, 1, 0.0, None) == 1


def test_quantile_positions_equal_the_f64_arithmetic():
    for n in (1, 2, 3, 10, 2 ** 53 + 1):
        for q in (0.0, 0.25, 0.5, 0.999, 1.0):
            p = np.float64(q) * np.float64(n - 1)
            expected = (int(np.floor(p)), int(np.ceil(p)), float(p - np.floor(p)))
            assert mdb.quantile_positions(q, n) == expected, (n, q)
            assert 0 <= expected[0] <= expected[1] <= n - 1
    for q, n in ((0.5, 0), (-1e-9, 5), (1.0 + 1e-9, 5), (math.nan, 5), (math.inf, 5)):
        with pytest.raises(mdb.HipError):
            mdb.quantile_positions(q, n)
    library = mdb.load_hip_library()
    assert library.mdb_quantile_positions(0.5, 5, None, None, None) == 1


def test_hist_request_layout_agrees_everywhere():
    text = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    size = re.search(r"MDB_LAYOUT_ASSERT\(sizeof\(mdb_hist_request\) == (\d+)\)", text)
    offsets = re.findall(r"MDB_LAYOUT_ASSERT\(offsetof\(mdb_hist_request, (\w+)\) == (\d+)\)", text)
    assert size and int(size.group(1)) == 32 == ctypes.sizeof(_abi.HistRequestC)
    assert {field for field, _ in offsets} == {name for name, _ in _abi.HistRequestC._fields_} - {"t_lo"}
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    assert re.search(r"size_of::<mdb_hist_request>\(\) == 32\b", rust)
    for field, offset in offsets:
        assert getattr(_abi.HistRequestC, field).offset == int(offset), field
        assert re.search(rf"offset_of!\(mdb_hist_request, {field}\) == {offset}\b", rust), field
    assert [getattr(_abi.HistRequestC, name).offset for name, _ in _abi.HistRequestC._fields_] == [0, 8, 16, 20, 24, 28]
    struct_text = re.search(r"typedef struct mdb_hist_request \{(.*?)\} mdb_hist_request;", text, re.S).group(1)
    header_fields = re.findall(r"\b(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", struct_text, flags=re.S))
    header_names = [name for pair in header_fields for name in pair if name]
    assert header_names == [name for name, _ in _abi.HistRequestC._fields_]
    rust_struct = re.search(r"pub struct mdb_hist_request \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+):", rust_struct) == header_names
    assert re.search(r"#define MDB_HIST_MAX_EDGES\s+4095u", text) and _abi.MDB_HIST_MAX_EDGES == 4095
    assert re.search(r"pub const MDB_HIST_MAX_EDGES: u32 = 4095;", rust)


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


def test_requests_are_checked_before_the_device_is_used():
    """No GPU is needed to be told that a request is malformed: the checks come before the context is touched (the
    context pointer handed in here is never dereferenced)."""
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)
    pattern = np.full(4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    good_edges = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    bad_requests = [(_abi.HistRequestC(0, 10, 3, 1, 1, 0), good_edges), (_abi.HistRequestC(0, 10, 3, 1, 0, 1), good_edges),
                    (_abi.HistRequestC(0, 10, 0, 1, 0, 0), good_edges), (_abi.HistRequestC(0, 10, 4096, 1, 0, 0), good_edges),
                    (_abi.HistRequestC(0, 10, 3, 0, 0, 0), good_edges),
                    (_abi.HistRequestC(0, 10, 3, 1, 0, 0), np.array([1.0, 1.0, 3.0], dtype=np.float32)),
                    (_abi.HistRequestC(0, 10, 3, 1, 0, 0), np.array([3.0, 2.0, 1.0], dtype=np.float32)),
                    (_abi.HistRequestC(0, 10, 2, 1, 0, 0), _f32([0x00000000, 0x80000000]))]
    for request, edges in bad_requests:
        counts = pattern.copy()
        for call in (library.mdb_hist_batch, library.mdb_hist_batch_dev):
            assert call(fake_context, ctypes.byref(seg), None, ctypes.byref(request), edges.ctypes.data,
                        counts.ctypes.data) == 1
        pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
        assert library.mdb_hist_batch_list(fake_context, pointers, None, 1, ctypes.byref(request), edges.ctypes.data,
                                           counts.ctypes.data) == 1
        assert np.array_equal(counts, pattern)
    lo, hi = np.full(2, 7.0, dtype=np.float32), np.full(2, 7.0, dtype=np.float32)
    n_points = ctypes.c_uint64(99)
    for q, n_q in ((np.array([0.5, 1.5]), 2), (np.array([math.nan, 0.5]), 2), (np.array([0.5, -0.1]), 2),
                   (np.array([0.5, 0.5]), 0), (np.full(17, 0.5), 17)):
        for call in (library.mdb_quantile_batch, library.mdb_quantile_batch_dev):
            assert call(fake_context, ctypes.byref(seg), 0, 10, q.ctypes.data, n_q, lo.ctypes.data, hi.ctypes.data,
                        ctypes.byref(n_points)) == 1
        assert n_points.value == 99 and (lo == 7.0).all() and (hi == 7.0).all()
    # NULL arguments
    request = _abi.HistRequestC(0, 10, 3, 1, 0, 0)
    assert library.mdb_hist_batch(None, None, None, None, None, None) == 1
    assert library.mdb_hist_batch_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(request), None,
                                      pattern.ctypes.data) == 1
    assert library.mdb_hist_batch_list(fake_context, None, None, 1, ctypes.byref(request), good_edges.ctypes.data,
                                       pattern.ctypes.data) == 1
    assert library.mdb_quantile_batch(fake_context, ctypes.byref(seg), 0, 10, None, 1, lo.ctypes.data, hi.ctypes.data,
                                      ctypes.byref(n_points)) == 1
    assert b"NULL" in library.mdb_last_error()


@pytest.fixture(scope="module")
def built():
    done = subprocess.run(["make", "-C", HERE, "all"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


@pytest.mark.parametrize("flavour", ["plain", "asan"])
def test_refinement_pins_every_order_statistic_without_a_gpu(built, flavour):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    done = subprocess.run([os.path.join(HERE, "_build", f"check_{flavour}")], capture_output=True, text=True, env=env,
                          timeout=300)
    output = done.stdout + done.stderr
    assert done.returncode == 0, output[-4000:]
    assert output.startswith("ok: ") or "\nok: " in output, output[-4000:]
    for report in ("ERROR: AddressSanitizer", "runtime error:", "MISMATCH"):
        assert report not in output, output[-4000:]
