"""CPU-side checks of the row masks' ABI: the six entry points in the built library, the header, the Rust binding and
the ctypes table; the MDB_MASK_* operations with the same numbers in all three; and the bit layout of a mask on the
host (download_mask / unpack_mask / upload_mask's packing) against bitmaps made by hand."""

import os
import re
import subprocess

import numpy as np
import pytest

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi, api

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdb_mask_filter_dev", "mdb_mask_combine_dev", "mdb_grid_batch_mask_dev", "mdb_agg_batch_mask_dev",
         "mdb_agg_batch_where", "mdb_grid_batch_where_owned")
OPS = (("AND", 0), ("OR", 1), ("XOR", 2), ("ANDNOT", 3), ("NOT", 4))


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


def test_mask_operations_agree_in_header_ctypes_and_rust():
    header = open(os.path.join(REPO_ROOT, "include", "mdb.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    for name, value in OPS:
        assert re.search(rf"#define MDB_MASK_{name}\s+{value}u\b", header), name
        assert getattr(_abi, f"MDB_MASK_{name}") == value == getattr(mdb, f"MDB_MASK_{name}")
        assert re.search(rf"pub const MDB_MASK_{name}: u32 = {value};", rust), name
    assert len(re.findall(r"#define MDB_MASK_\w+", header)) == len(OPS)


def test_context_methods_exist():
    for method in ("mask_filter_dev", "mask_combine_dev", "grid_mask_dev", "grid_mask_resident", "agg_mask_dev",
                   "agg_where", "grid_where", "download_mask", "upload_mask"):
        assert callable(getattr(api.Context, method)), method


class _Memory:
    """Stands in for a context: `download_array` / `upload_array` over a bytes object instead of the device."""

    def __init__(self, raw=b""):
        self.raw = np.frombuffer(raw, dtype=np.uint8)

    def download_array(self, pointer, count, dtype):
        assert pointer == 4096
        return self.raw[:count * np.dtype(dtype).itemsize].view(dtype).copy()

    def upload_array(self, array):
        self.raw = np.ascontiguousarray(array).view(np.uint8).copy()
        return 4096


@pytest.mark.parametrize("n_rows", [1, 7, 8, 9, 63, 64, 65, 77, 128, 129, 1000])
def test_download_mask_reads_row_r_from_bit_r_mod_64_of_word_r_div_64(n_rows):
    rng = np.random.default_rng(n_rows)
    rows = rng.random(n_rows) < 0.4
    rows[-1] = True
    words = [0] * mdb.mask_words(n_rows)
    for r in np.flatnonzero(rows).tolist():  # the layout of mdb.h, by hand
        words[r // 64] |= 1 << (r % 64)
    raw = b"".join(int(word).to_bytes(8, "little") for word in words)
    assert mdb.mask_words(n_rows) == -(-n_rows // 64) and len(raw) == 8 * mdb.mask_words(n_rows)
    memory = _Memory(raw)
    got = api.Context.download_mask(memory, 4096, n_rows)
    assert got.dtype == np.bool_ and got.shape == (n_rows,) and np.array_equal(got, rows)
    padded = api.Context.download_mask(memory, 4096, n_rows, with_padding=True)
    assert len(padded) == 64 * len(words) and np.array_equal(padded[:n_rows], rows) and not padded[n_rows:].any()
    assert np.array_equal(mdb.unpack_mask(np.frombuffer(raw, dtype=np.uint8), n_rows), rows)
    # an Arrow boolean bitmap byte for byte: bit r % 8 of byte r / 8
    for r in (0, n_rows // 2, n_rows - 1):
        assert bool(raw[r // 8] >> (r % 8) & 1) == bool(rows[r])
    # and upload_mask packs the same bytes, the padding bits zero
    packer = _Memory()
    assert api.Context.upload_mask(packer, rows) == 4096
    assert packer.raw.tobytes() == raw


def test_download_mask_of_no_rows():
    assert mdb.mask_words(0) == 0
    assert len(api.Context.download_mask(_Memory(), 4096, 0)) == 0
