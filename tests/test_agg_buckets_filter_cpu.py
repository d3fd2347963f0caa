"""CPU-side checks of the filtered bucket aggregates (mdb_agg_buckets_filter*): the three entry points in the header, the
ctypes mirror, the built library's exports, the Rust binding and the Python methods."""

import ctypes
import inspect
import os
import re

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdb_agg_buckets_filter", "mdb_agg_buckets_filter_dev", "mdb_agg_buckets_filter_list")


def _read(*parts):
    with open(os.path.join(REPO_ROOT, *parts)) as f:
        return f.read()


def test_entry_points_are_declared_mirrored_and_exported():
    header = _read("include", "mdb.h")
    for name in NAMES:
        declaration = re.search(rf"\bint {name}\((.*?)\);", header, re.S)
        assert declaration, name
        assert "const mdb_value_filter *filter" in declaration.group(1), name
        assert "const mdb_bucket_request *request" in declaration.group(1), name
        assert name in _abi.hip_symbol_names(), name
    library = ctypes.CDLL(_abi.HIP_LIBRARY_PATH)  # (dlsym: only what the library exports)
    for name in NAMES:
        assert hasattr(library, name), name


def test_ctypes_prototypes_take_the_filter_after_the_request():
    request, flt = ctypes.POINTER(_abi.BucketRequestC), ctypes.POINTER(_abi.ValueFilterC)
    for name in NAMES:
        _, argtypes = _abi._HIP_SYMBOLS[name]
        assert request in argtypes and flt in argtypes, name
        assert argtypes.index(flt) == argtypes.index(request) + 1, name


def test_rust_declares_the_entry_points_and_the_methods():
    sys_rs = _read("rust", "modelardb_hip", "src", "sys.rs")
    for name in NAMES:
        declaration = re.search(rf"pub fn {name}\((.*?)\) -> c_int;", sys_rs, re.S)
        assert declaration, name
        assert re.search(r"filter: \*const mdb_value_filter", declaration.group(1)), name
        assert re.search(r"request: \*const mdb_bucket_request", declaration.group(1)), name
    lib_rs = _read("rust", "modelardb_hip", "src", "lib.rs")
    for method, call in (("agg_buckets_filter", "mdb_agg_buckets_filter"),
                         ("agg_buckets_filter_list", "mdb_agg_buckets_filter_list")):
        assert re.search(rf"pub fn {method}\(", lib_rs), method
        assert re.search(rf"sys::{call}\(", lib_rs), call


def test_python_methods_mirror_agg_buckets():
    expected = ["self", "flt", "origin", "width", "n_buckets", "groups", "t_lo", "t_hi", "which_mask", "states",
                "n_groups"]
    for name, first in (("agg_buckets_filter", "batch"), ("agg_buckets_filter_list", "batches"),
                        ("agg_buckets_filter_dev", "dev_segments")):
        method = getattr(mdb.Context, name)
        parameters = inspect.signature(method).parameters
        assert list(parameters) == expected[:1] + [first] + expected[1:], name
        for default_none in ("groups", "t_lo", "t_hi", "states", "n_groups"):
            assert parameters[default_none].default is None, (name, default_none)
        assert parameters["which_mask"].default == (mdb.MDB_AGG_COUNT | mdb.MDB_AGG_MIN | mdb.MDB_AGG_MAX
                                                    | mdb.MDB_AGG_SUM)
