"""CPU-side checks of the bucketed aggregates' ABI: mdb_agg_merge_n (host arithmetic, no context) and the layout of
mdb_bucket_request in the header, the ctypes mirror and the Rust binding."""

import ctypes
import os
import re

import numpy as np

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_states(rng, n):
    states = mdb.fresh_agg_states(n)
    kind = rng.integers(0, 6, n)
    states["sum"] = np.where(kind == 1, np.inf, rng.normal(size=n) * 10.0 ** rng.integers(-3, 30, n))
    states["count"] = rng.integers(0, 1 << 40, n)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45], dtype=np.float32)
    for field in ("min", "max"):
        values = rng.normal(size=n).astype(np.float32) * np.float32(1e3)
        values = np.where(kind == 2, specials[rng.integers(0, len(specials), n)], values)
        states[field] = np.where(kind == 0, states[field], values)  # kind 0: a fresh state
    states["sum"][kind == 0], states["count"][kind == 0] = 0.0, 0
    states["min"][kind == 3] = np.nan  # NaN minima (a NaN-only cell of a reference state)
    return states


def test_merge_n_equals_n_merges():
    lib = _abi.load_hip_library()
    rng = np.random.default_rng(17)
    for n in (1, 2, 7, 1000):
        into, other = _random_states(rng, n), _random_states(rng, n)
        expected = into.copy()
        for k in range(n):
            state = _abi.AggStateC(*[expected[k][field].item() for field in ("sum", "count", "min", "max")])
            source = _abi.AggStateC(*[other[k][field].item() for field in ("sum", "count", "min", "max")])
            assert lib.mdb_agg_merge(ctypes.byref(state), ctypes.byref(source)) == 0
            expected[k] = (state.sum, state.count, state.min, state.max)
        got = mdb.agg_merge_n(into, other)
        assert got.tobytes() == expected.tobytes()


def test_merge_n_of_nothing_succeeds():
    lib = _abi.load_hip_library()
    assert lib.mdb_agg_merge_n(None, None, 0) == 0
    empty = mdb.fresh_agg_states(0)
    assert mdb.agg_merge_n(empty, empty.copy()).size == 0
    assert lib.mdb_agg_merge_n(None, None, 1) != 0  # but NULL arrays of one state are an error


def test_bucket_request_layout_agrees_everywhere():
    text = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    size = re.search(r"MDB_LAYOUT_ASSERT\(sizeof\(mdb_bucket_request\) == (\d+)\)", text)
    offsets = re.findall(r"MDB_LAYOUT_ASSERT\(offsetof\(mdb_bucket_request, (\w+)\) == (\d+)\)", text)
    assert size and int(size.group(1)) == 48 == ctypes.sizeof(_abi.BucketRequestC)
    assert {field for field, _ in offsets} == {name for name, _ in _abi.BucketRequestC._fields_} - {"origin"}
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    assert re.search(r"size_of::<mdb_bucket_request>\(\) == 48\b", rust)
    for field, offset in offsets:
        assert getattr(_abi.BucketRequestC, field).offset == int(offset), field
        assert re.search(rf"offset_of!\(mdb_bucket_request, {field}\) == {offset}\b", rust), field
    # the fields in one order, with one width, in all three
    struct = re.search(r"typedef struct mdb_bucket_request \{(.*?)\} mdb_bucket_request;", text, re.S).group(1)
    header_fields = re.findall(r"\b(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    header_names = [name for pair in header_fields for name in pair if name]
    assert header_names == [name for name, _ in _abi.BucketRequestC._fields_]
    rust_struct = re.search(r"pub struct mdb_bucket_request \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+):", rust_struct) == header_names
    for name in ("mdb_agg_buckets", "mdb_agg_buckets_dev", "mdb_agg_buckets_list", "mdb_agg_merge_n"):
        assert name in _abi.hip_symbol_names() and re.search(rf"pub fn {name}\(", rust)
