"""CPU-side checks of the value filters' ABI: the layout of mdb_value_filter in the header, the ctypes mirror and the
Rust binding, the six entry points in the built library, and the exact conversion of f64 literals into f32
totalOrder bounds by mdb.value_filter, against a numpy brute force."""

import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdb_grid_count_filter_dev", "mdb_grid_batch_filter_dev", "mdb_grid_batch_filter_owned",
         "mdb_agg_batch_filter", "mdb_agg_batch_filter_dev", "mdb_agg_batch_filter_list")


def test_value_filter_layout_agrees_everywhere():
    text = open(os.path.join(REPO_ROOT, "include", "mdb_format.h")).read()
    size = re.search(r"MDB_LAYOUT_ASSERT\(sizeof\(mdb_value_filter\) == (\d+)\)", text)
    offsets = re.findall(r"MDB_LAYOUT_ASSERT\(offsetof\(mdb_value_filter, (\w+)\) == (\d+)\)", text)
    assert size and int(size.group(1)) == 32 == ctypes.sizeof(_abi.ValueFilterC)
    assert {field for field, _ in offsets} == {name for name, _ in _abi.ValueFilterC._fields_} - {"t_lo"}
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    assert re.search(r"size_of::<mdb_value_filter>\(\) == 32\b", rust)
    for field, offset in offsets:
        assert getattr(_abi.ValueFilterC, field).offset == int(offset), field
        assert re.search(rf"offset_of!\(mdb_value_filter, {field}\) == {offset}\b", rust), field
    struct_text = re.search(r"typedef struct mdb_value_filter \{(.*?)\} mdb_value_filter;", text, re.S).group(1)
    header_fields = re.findall(r"\b(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", struct_text, flags=re.S))
    header_names = [name for pair in header_fields for name in pair if name]
    assert header_names == [name for name, _ in _abi.ValueFilterC._fields_]
    rust_struct = re.search(r"pub struct mdb_value_filter \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+):", rust_struct) == header_names
    for flag, value in (("LO_OPEN", 1), ("HI_OPEN", 2), ("NO_LO", 4), ("NO_HI", 8)):
        assert re.search(rf"#define MDB_VALUE_{flag}\s+{value}u", text), flag
        assert getattr(_abi, f"MDB_VALUE_{flag}") == value
        assert re.search(rf"pub const MDB_VALUE_{flag}: u32 = {value};", rust), flag


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


# ---- the converter ----------------------------------------------------------------------------------------------

def _key32(bits):
    bits = np.asarray(bits, dtype=np.uint32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def _key64_of_f32_bits(bits):
    """f64 totalOrder key of float(v) for f32 bit patterns (NaN payloads moved up by 29 bits, as the conversion does)."""
    out = []
    for b in np.asarray(bits, dtype=np.uint32).tolist():
        if (b >> 23) & 0xFF == 0xFF and b & 0x7FFFFF:
            wide = ((b >> 31) << 63) | (0x7FF << 52) | ((b & 0x7FFFFF) << 29)
        else:
            wide = struct.unpack("<Q", struct.pack("<d", struct.unpack("<f", struct.pack("<I", b))[0]))[0]
        signed = wide - (1 << 64) if wide >> 63 else wide
        out.append(signed ^ ((signed >> 63) & 0x7FFFFFFFFFFFFFFF))
    return np.array(out, dtype=object)


def _key64(x):
    signed = struct.unpack("<q", struct.pack("<d", x))[0]
    return signed ^ ((signed >> 63) & 0x7FFFFFFFFFFFFFFF)


def _selected(flt, bits):
    """What the library selects (mdb_format.h): closed key bounds from the flags, keys compared as integers."""
    lo_bits, hi_bits = mdb.value_filter_bits(flt)
    lo = -(1 << 31) if flt.flags & 4 else int(_key32([lo_bits])[0]) + (1 if flt.flags & 1 else 0)
    hi = (1 << 31) - 1 if flt.flags & 8 else int(_key32([hi_bits])[0]) - (1 if flt.flags & 2 else 0)
    keys = _key32(bits)
    return (keys >= lo) & (keys <= hi)


def _f32_bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


def _literals():
    nan_neg = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
    nan_payload = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000001))[0]  # not an f32 NaN
    nan_low = struct.unpack("<d", struct.pack("<Q", 0x7FF0000020000000))[0]      # f32 sNaN 0x7f800001 widened
    out = [0.0, -0.0, math.inf, -math.inf, math.nan, nan_neg, nan_payload, nan_low, 1.0, -1.0, 30.0, 0.1, -0.1, 1e-40,
           -1e-40, 1e-45, 7e-46, 1.4e-45, 3.4028234663852886e38, 3.5e38, -3.5e38, 1e300, -1e300, 5e-324, 100.0 + 1e-9,
           2.0 ** -149, 2.0 ** -150, 1.1754942e-38, 16777217.0]
    return out


def _values():
    """f32 bit patterns: ±0, ±inf, NaN of both signs and several payloads, subnormals, and every literal's f32
    neighbours (two on each side of its nearest f32)."""
    base = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,
            0x7FFFFFFF, 0xFFFFFFFF, 0x7FC00001, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000,
            0x7F7FFFFF, 0xFF7FFFFF]
    for c in _literals():
        if math.isnan(c):
            continue
        with np.errstate(over="ignore"):
            nearest = int(np.float32(c).view(np.uint32))
        key = int(_key32([nearest])[0])
        for d in range(-2, 3):
            k = max(-(1 << 31), min((1 << 31) - 1, key + d))
            base.append((k ^ ((k >> 31) & 0x7FFFFFFF)) & 0xFFFFFFFF)
    return np.unique(np.array(base, dtype=np.uint32))


@pytest.mark.parametrize("op", [">=", ">", "<=", "<"])
def test_converter_matches_f64_total_order(op):
    bits = _values()
    value_keys = _key64_of_f32_bits(bits)
    for c in _literals():
        k = _key64(c)
        if op == ">=":
            flt, expected = mdb.value_filter(lo=c), value_keys >= k
        elif op == ">":
            flt, expected = mdb.value_filter(lo=c, lo_open=True), value_keys > k
        elif op == "<=":
            flt, expected = mdb.value_filter(hi=c), value_keys <= k
        else:
            flt, expected = mdb.value_filter(hi=c, hi_open=True), value_keys < k
        got = _selected(flt, bits)
        assert np.array_equal(got, expected.astype(bool)), (op, c, bits[got != expected.astype(bool)])


def test_converter_between_and_empty_intervals():
    bits = _values()
    value_keys = _key64_of_f32_bits(bits)
    literals = _literals()
    for lo in literals:
        for hi in literals[::3]:
            for lo_open in (False, True):
                for hi_open in (False, True):
                    flt = mdb.value_filter(lo=lo, hi=hi, lo_open=lo_open, hi_open=hi_open)
                    lo_ok = value_keys > _key64(lo) if lo_open else value_keys >= _key64(lo)
                    hi_ok = value_keys < _key64(hi) if hi_open else value_keys <= _key64(hi)
                    expected = (lo_ok & hi_ok).astype(bool)
                    assert np.array_equal(_selected(flt, bits), expected), (lo, hi, lo_open, hi_open)
    # [c, c) selects nothing, [c, c] exactly the f32 values equal to c in totalOrder
    assert not _selected(mdb.value_filter(lo=1.0, hi=1.0, hi_open=True), bits).any()
    same = _selected(mdb.value_filter(lo=-0.0, hi=-0.0), bits)
    assert set(bits[same].tolist()) == {0x80000000}


def test_converter_fields():
    flt = mdb.value_filter(lo=30.0, lo_open=True, t_lo=5, t_hi=9)
    assert (flt.t_lo, flt.t_hi, flt.reserved) == (5, 9, 0)
    assert flt.flags & mdb.MDB_VALUE_NO_HI and not flt.flags & mdb.MDB_VALUE_NO_LO
    assert mdb.value_filter_bits(flt)[0] == int(np.float32(30.0).view(np.uint32)) + 1  # the next f32 above 30
    everything = mdb.value_filter()
    assert everything.flags == mdb.MDB_VALUE_NO_LO | mdb.MDB_VALUE_NO_HI
    assert (everything.t_lo, everything.t_hi) == (-(1 << 63), (1 << 63) - 1)
