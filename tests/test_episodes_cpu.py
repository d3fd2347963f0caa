"""CPU-side checks of the episode operator (mdb_episodes*): the entry points in the built library, the header, the
ctypes mirror and the Rust binding; the two 64-byte structs; the request checks, made before the device is used; and
the run monoid and attribution rule of modelardb-rs_amd/csrc/mdb_episodes.hpp - the text the kernels compile - driven
by a stand-alone program against a row-by-row loop, plain and under AddressSanitizer + UBSan (tests/episodes_host)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO_ROOT, "tests", "episodes_host")
NAMES = ("mdb_episodes", "mdb_episodes_count_dev", "mdb_episodes_dev", "mdb_episodes_list", "mdb_episodes_result_free")


def test_entry_points_exported_declared_and_bound():
    library = _abi.HIP_LIBRARY_PATH
    assert os.path.exists(library), "build() first"
    exported = subprocess.run(["nm", "-D", "--defined-only", library], check=True, capture_output=True,
                              text=True).stdout.split()
    header = open(os.path.join(REPO_ROOT, "include", "mdb.h")).read()
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    wrappers = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in exported, name
        assert re.search(rf"\b(int|void) {name}\(", header), name
        assert re.search(rf"pub fn {name}\(", rust), name
        assert name in _abi.hip_symbol_names(), name
    declared = set(re.findall(r"\b(mdb_\w+)\(", header))
    listed = {name for name in exported if name.startswith("mdb_")}
    assert {name for name in declared | listed if "episodes" in name} == set(NAMES)
    for method in ("episodes", "episodes_list"):
        assert re.search(rf"pub fn {method}\(", wrappers), method
    for method in ("episodes", "episodes_list", "episodes_dev", "episodes_count_dev", "episodes_into_dev"):
        assert callable(getattr(mdb.Context, method)), method


def test_structs_are_64_bytes():
    header = open(os.path.join(REPO_ROOT, "include", "mdb.h")).read()
    for struct in ("mdb_episode", "mdb_episodes_request"):
        assert f"MDB_LAYOUT_ASSERT(sizeof({struct}) == 64);" in header
    assert ctypes.sizeof(_abi.EpisodeC) == 64 and ctypes.sizeof(_abi.EpisodesRequestC) == 64
    assert mdb.EPISODE_DTYPE.itemsize == 64
    for name, _ in _abi.EpisodeC._fields_:
        assert mdb.EPISODE_DTYPE.fields[name][1] == getattr(_abi.EpisodeC, name).offset, name
    assert _abi.EpisodesRequestC.max_gap.offset == 32 and _abi.EpisodesRequestC.n_groups.offset == 56
    rust = open(os.path.join(REPO_ROOT, "rust", "modelardb_hip", "src", "sys.rs")).read()
    for struct in ("mdb_episode", "mdb_episodes_request"):
        assert f"assert!(std::mem::size_of::<{struct}>() == 64)" in rust


def _request(flt=None, max_gap=0, min_duration=0, min_count=0, n_groups=1, flags=0):
    request = _abi.EpisodesRequestC()
    flt = flt or mdb.value_filter()
    ctypes.memmove(ctypes.addressof(request), ctypes.addressof(flt), ctypes.sizeof(flt))
    request.max_gap, request.min_duration, request.min_count = max_gap, min_duration, min_count
    request.n_groups, request.flags = n_groups, flags
    return request


def test_requests_are_checked_before_the_device_is_used():
    library = mdb.load_hip_library()
    batch = mdb.SegmentBatch.from_rows([(0, 100, 500, bytes([5]), 1.5, 1.5, b"", b"")])
    seg = batch.as_c()
    fake_context = ctypes.c_void_p(8)   # (never dereferenced)
    out = np.frombuffer(bytes([0xA5]) * (64 * 4), dtype=np.uint8).copy()
    counters = (ctypes.c_uint64 * 3)(11, 22, 33)
    result = ctypes.POINTER(_abi.EpisodesResultC)()
    pointers = (ctypes.POINTER(_abi.SegmentsC) * 1)(ctypes.pointer(seg))
    no_groups = (ctypes.c_void_p * 1)(None)
    bad_flags, bad_reserved = mdb.value_filter(), mdb.value_filter()
    bad_flags.flags = 64
    bad_reserved.reserved = 1

    def untouched():
        return (out.tobytes() == bytes([0xA5]) * (64 * 4) and list(counters) == [11, 22, 33] and not result)

    def calls(request, groups=None, group_pointers=no_groups):
        r, c = ctypes.byref(request), counters
        word = lambda k: ctypes.cast(ctypes.byref(c, 8 * k), ctypes.POINTER(ctypes.c_uint64))
        return (lambda: library.mdb_episodes_count_dev(fake_context, ctypes.byref(seg), groups, r, word(0), word(1), word(2)),
                lambda: library.mdb_episodes_dev(fake_context, ctypes.byref(seg), groups, r, out.ctypes.data, 4, word(0),
                                                 word(1), word(2)),
                lambda: library.mdb_episodes(fake_context, ctypes.byref(seg), groups, r, ctypes.byref(result)),
                lambda: library.mdb_episodes_list(fake_context, pointers, group_pointers, 1, r, ctypes.byref(result)))

    for request, message in ((_request(bad_flags), b"flag bits"), (_request(bad_reserved), b"reserved"),
                             (_request(flags=1), b"flags must be 0"), (_request(max_gap=-1), b"max_gap"),
                             (_request(min_duration=-5), b"min_duration"), (_request(n_groups=0), b"n_groups")):
        for call in calls(request):
            assert call() == 1
            assert message in library.mdb_last_error()
        assert untouched()
    # a bad group id of a host form is found on the host
    groups = np.array([3], dtype=np.uint32)
    group_pointers = (ctypes.c_void_p * 1)(groups.ctypes.data)
    for call in calls(_request(n_groups=3), groups.ctypes.data, group_pointers)[2:]:
        assert call() == 1 and b"group id" in library.mdb_last_error()
    assert untouched()
    good = _request()
    word = ctypes.cast(counters, ctypes.POINTER(ctypes.c_uint64))
    for call in (lambda: library.mdb_episodes_count_dev(None, ctypes.byref(seg), None, ctypes.byref(good), word, word, word),
                 lambda: library.mdb_episodes_count_dev(fake_context, None, None, ctypes.byref(good), word, word, word),
                 lambda: library.mdb_episodes_count_dev(fake_context, ctypes.byref(seg), None, None, word, word, word),
                 lambda: library.mdb_episodes_count_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(good), None, word, word),
                 lambda: library.mdb_episodes_dev(fake_context, ctypes.byref(seg), None, ctypes.byref(good), out.ctypes.data, 4,
                                                  word, None, word),
                 lambda: library.mdb_episodes(fake_context, None, None, ctypes.byref(good), ctypes.byref(result)),
                 lambda: library.mdb_episodes(fake_context, ctypes.byref(seg), None, ctypes.byref(good), None),
                 lambda: library.mdb_episodes_list(fake_context, None, no_groups, 1, ctypes.byref(good), ctypes.byref(result)),
                 lambda: library.mdb_episodes_list(fake_context, pointers, no_groups, 1, None, ctypes.byref(result))):
        assert call() == 1 and b"NULL" in library.mdb_last_error()
    assert untouched()
    # nothing to do: an empty list succeeds without a context that could be used
    assert library.mdb_episodes_list(fake_context, pointers, no_groups, 0, ctypes.byref(good), ctypes.byref(result)) == 0
    assert result and result.contents.n == 0 and result.contents.n_rows == 0 and result.contents.n_passing == 0
    library.mdb_episodes_result_free(result)


@pytest.fixture(scope="module")
def built():
    done = subprocess.run(["make", "-C", HERE, "all"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "warning" not in done.stdout + done.stderr, done.stdout + done.stderr


@pytest.mark.parametrize("flavour", ["plain", "asan"])
def test_monoid_and_attribution_without_a_gpu(built, flavour):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    done = subprocess.run([os.path.join(HERE, "_build", f"check_{flavour}")], capture_output=True, text=True, env=env,
                          timeout=300)
    output = done.stdout + done.stderr
    assert done.returncode == 0, output[-4000:]
    assert output.startswith("ok: ") or "\nok: " in output, output[-4000:]
    for report in ("ERROR: AddressSanitizer", "runtime error:", "MISMATCH"):
        assert report not in output, output[-4000:]
