"""CPU-side checks of the variance operator (mdb_moments_buckets*, mdb_moments_merge_n, mdb_moments_variance): the
entry points in the built library, the header, the ctypes mirror and the Rust binding; the layout of mdb_moments_cell
everywhere; mdb_moments_merge_n against the exact reference of tests/test_gpu_moments.py on random splits;
mdb_moments_variance; and the host side (modelardb-rs_amd/csrc/mdb_moments_host.cpp) driven by a stand-alone program,
plain and under AddressSanitizer + UBSan (tests/moments_host)."""

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
HERE = os.path.join(REPO_ROOT, "tests", "moments_host")
NAMES = ("mdb_moments_buckets", "mdb_moments_buckets_dev", "mdb_moments_buckets_list", "mdb_moments_merge_n",
         "mdb_moments_variance")
OFFSETS = {"count": 0, "mean": 8, "m2": 16}
MEAN_TOLERANCE = 2.0 ** -44   # of the largest |v|
M2_TOLERANCE = 1e-5           # of m2_ref


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


def test_cell_layout_agrees_everywhere():
    assert ctypes.sizeof(_abi.MomentsCellC) == 24 == mdb.MOMENTS_CELL_DTYPE.itemsize
    assert [name for name, _ in _abi.MomentsCellC._fields_] == list(OFFSETS) == list(mdb.MOMENTS_CELL_DTYPE.names)
    text = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    assert re.search(r"MDB_LAYOUT_ASSERT\(sizeof\(mdb_moments_cell\) == 24\)", text)
    assert re.search(r"size_of::<mdb_moments_cell>\(\) == 24\b", rust)
    for name, offset in OFFSETS.items():
        assert getattr(_abi.MomentsCellC, name).offset == offset == mdb.MOMENTS_CELL_DTYPE.fields[name][1], name
        if offset:
            assert re.search(rf"MDB_LAYOUT_ASSERT\(offsetof\(mdb_moments_cell, {name}\) == {offset}\)", text), name
            assert re.search(rf"offset_of!\(mdb_moments_cell, {name}\) == {offset}\b", rust), name
    rust_struct = re.search(r"pub struct mdb_moments_cell \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", rust_struct) == [("count", "i64"), ("mean", "f64"), ("m2", "f64")]
    c_struct = re.search(r"typedef struct mdb_moments_cell \{(.*?)\} mdb_moments_cell;", text, re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", c_struct) == [("int64_t", "count"), ("double", "mean"), ("double", "m2")]
    assert mdb.fresh_moments_cells((2, 3)).tobytes() == bytes(6 * 24)


def _reference(values):
    """(mean_ref, m2_ref) of f32 values in exact arithmetic: the reference of tests/test_gpu_moments.py."""
    d = values.astype(np.float64) - float(values[0])
    shift = math.fsum(d) / len(d)
    return float(values[0]) + shift, math.fsum((d - shift) ** 2)


def _cells_of(runs):
    cells = mdb.fresh_moments_cells(len(runs))
    for k, run in enumerate(runs):
        if len(run):
            cells[k] = (len(run),) + _reference(run)
    return cells


def _data_sets(rng, n):
    low = np.float32(1.0e7)
    return {
        "level_1e6_sigma_0.5": (1.0e6 + rng.normal(0.0, 0.5, n)).astype(np.float32),
        "standard_normal": rng.normal(0.0, 1.0, n).astype(np.float32),
        "ramp": (-250.0 + 0.03125 * np.arange(n)).astype(np.float32),
        "level_1e7_one_ulp": np.where(rng.random(n) < 0.5, low, np.nextafter(low, np.float32(np.inf))).astype(np.float32),
        "constant": np.full(n, 1234.567, dtype=np.float32),
    }


def test_merge_on_random_splits_meets_the_tolerance():
    """Every data set cut at random places into runs (some empty), each run's cell exact, the runs merged one after
    the other into the first: count exact, mean within 2^-44 of the largest |v|, m2 within 1e-5 of m2_ref - 0.0
    exactly for the constant one."""
    rng = np.random.default_rng(2030)
    for name, values in _data_sets(rng, 20_000).items():
        mean_ref, m2_ref = _reference(values)
        largest = float(np.abs(values.astype(np.float64)).max())
        for n_runs in (2, 29, 400, 2858):
            cuts = np.sort(rng.integers(0, len(values) + 1, n_runs - 1))
            runs = np.split(values, cuts)
            assert n_runs < 100 or any(len(run) == 0 for run in runs)
            cells = _cells_of(runs)
            for order in (range(1, n_runs), list(rng.permutation(np.arange(1, n_runs)))):
                into = cells[:1].copy()
                for k in order:
                    mdb.moments_merge(into, cells[k:k + 1])
                assert into["count"][0] == len(values)
                assert abs(into["mean"][0] - mean_ref) <= MEAN_TOLERANCE * largest, (name, n_runs)
                assert abs(into["m2"][0] - m2_ref) <= M2_TOLERANCE * m2_ref, (name, n_runs, into["m2"][0], m2_ref)
                if name == "constant":
                    assert into["m2"][0] == 0.0 and into["mean"][0] == float(values[0])


def test_merge_is_the_documented_rule_cell_by_cell():
    rng = np.random.default_rng(2031)
    a, b = mdb.fresh_moments_cells(5_000), mdb.fresh_moments_cells(5_000)
    for cells in (a, b):
        cells["count"] = rng.integers(0, 4, len(cells)) * rng.integers(1, 1 << 40, len(cells))
        cells["mean"] = rng.normal(0.0, 1e3, len(cells))
        cells["m2"] = rng.random(len(cells)) * 1e6
    assert ((a["count"] == 0) & (b["count"] > 0)).any() and ((b["count"] == 0) & (a["count"] > 0)).any()
    got = mdb.moments_merge(a.copy(), b)
    na, nb = a["count"].astype(np.float64), b["count"].astype(np.float64)
    n = (a["count"] + b["count"]).astype(np.float64)
    d = b["mean"] - a["mean"]
    with np.errstate(invalid="ignore", divide="ignore"):
        expected = mdb.fresh_moments_cells(len(a))
        expected["count"] = a["count"] + b["count"]
        expected["mean"] = a["mean"] + d * (nb / n)
        expected["m2"] = a["m2"] + b["m2"] + d * d * (na * nb / n)
    expected[a["count"] == 0] = b[a["count"] == 0]
    expected[b["count"] == 0] = a[b["count"] == 0]
    assert got.tobytes() == expected.tobytes()


def test_a_fresh_cell_on_either_side_returns_the_other_sides_bytes():
    rng = np.random.default_rng(2032)
    cells = np.frombuffer(rng.bytes(24 * 2_000), dtype=mdb.MOMENTS_CELL_DTYPE).copy()
    cells["count"] = np.abs(cells["count"] >> 2) + 1   # (not empty; mean and m2 any bit pattern, NaNs among them)
    assert mdb.moments_merge(mdb.fresh_moments_cells(len(cells)), cells).tobytes() == cells.tobytes()
    assert mdb.moments_merge(cells.copy(), mdb.fresh_moments_cells(len(cells))).tobytes() == cells.tobytes()
    # count == 0: no other member is read - a cell of 0xA5 bytes with count 0 is empty
    stale = np.frombuffer(bytes([0xA5]) * (24 * len(cells)), dtype=mdb.MOMENTS_CELL_DTYPE).copy()
    stale["count"] = 0
    untouched = stale.copy()
    assert mdb.moments_merge(stale, mdb.fresh_moments_cells(len(cells))).tobytes() == untouched.tobytes()
    assert mdb.moments_merge(stale, cells).tobytes() == cells.tobytes()
    with pytest.raises(ValueError):
        mdb.moments_merge(cells, cells[:5])


def test_variance_for_both_ddof():
    cells = mdb.fresh_moments_cells(5)
    cells[1] = (1, 5.0, 0.0)
    cells[2] = (2, 1.5, 0.5)
    cells[3] = (10, -3.0, 90.0)
    cells[4] = (3, float("nan"), float("inf"))
    population, sample = mdb.moments_variance(cells, 0), mdb.moments_variance(cells, 1)
    assert np.isnan(population[0]) and population[1] == 0.0 and population[2] == 0.25 and population[3] == 9.0
    assert np.isnan(sample[0]) and np.isnan(sample[1]) and sample[2] == 0.5 and sample[3] == 10.0
    assert population[4] == float("inf") and sample[4] == float("inf")
    assert mdb.moments_variance(cells.reshape(5, 1), 1).shape == (5, 1)
    rng = np.random.default_rng(2033)
    values = rng.normal(50.0, 3.0, 1000).astype(np.float32)
    cell = _cells_of([values])
    for ddof in (0, 1):
        assert abs(mdb.moments_variance(cell, ddof)[0] - np.var(values.astype(np.float64), ddof=ddof)) < 1e-9
    for ddof in (2, 7):
        with pytest.raises(mdb.HipError, match="ddof"):
            mdb.moments_variance(cells, ddof)
    library = mdb.load_hip_library()
    out = np.full(5, 77.0)
    assert library.mdb_moments_variance(cells.ctypes.data, 5, 2, out.ctypes.data) == 1 and (out == 77.0).all()
    assert library.mdb_moments_variance(None, 1, 0, out.ctypes.data) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_moments_variance(None, 0, 0, None) == 0


def test_requests_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    cells = np.frombuffer(bytes([0xA5]) * (24 * 4), dtype=mdb.MOMENTS_CELL_DTYPE).copy()
    before = cells.copy()
    lo, hi = -(1 << 63), (1 << 63) - 1
    for request, message in ((_abi.BucketRequestC(0, 100, 4, lo, hi, 1, 1), b"which_mask"),
                             (_abi.BucketRequestC(0, 0, 4, lo, hi, 1, 0), b"width"),
                             (_abi.BucketRequestC(0, 100, 4, lo, hi, 0, 0), b"n_groups must"),
                             (_abi.BucketRequestC(0, 100, (1 << 64) // 8, lo, hi, 4_000_000_000, 0), b"overflows")):
        pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
        for call in (lambda: library.mdb_moments_buckets(fake_context, ctypes.byref(seg), None, ctypes.byref(request), cells.ctypes.data),
                     lambda: library.mdb_moments_buckets_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(request), cells.ctypes.data),
                     lambda: library.mdb_moments_buckets_list(fake_context, pointers, None, 1, ctypes.byref(request), cells.ctypes.data)):
            assert call() == 1
            assert message in library.mdb_last_error()
        assert cells.tobytes() == before.tobytes()
    assert library.mdb_moments_buckets(None, None, None, None, None) == 1 and b"NULL" in library.mdb_last_error()
    assert library.mdb_moments_merge_n(None, cells.ctypes.data, 1) == 1 and b"NULL" in library.mdb_last_error()


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
