"""The reduction tree and the fold every per-bucket operator shares (csrc/mdb_bucket_fold.hpp), through the
instantiations whose own tests do not run one run of equal keys through every level of the tree: integral, change,
sample and trend. (agg, m4, moments, comoments and binned have test_runs_of_one_cell_through_every_level_of_the_
reduction_tree in their own files.) Beside them, for agg and moments: runs of 63, 64 and 65 pairs, which end before,
on and behind the border of a 64-entry tile.

The data: one short series with segments of 2..12 rows, tiled with take() to a little over 4 096 segments - inside
every copy a segment's last row is linked to its right neighbour's first, between copies time runs backwards and the
link is broken. One bucket and one group: ONE run of more than 64^2 pairs, folded in pair order through levels 0, 1 and
2. Two buckets: the keys go 0 .. 0 1 .. 1 in every copy, so they are sorted and the fold walks order[].

Every result is held to the operator's own reference at that reference's own tolerance (integral_cases, change_cases,
sample_cases, trend_cases with comoments_cases.assert_cells, moments_cases, test_gpu_agg_buckets' grid oracle); the
integer members are exact there. The host form and the _dev form must agree byte for byte."""

import numpy as np
import pytest

import cases
import change_cases as chc
import comoments_cases as cc
import integral_cases as ic
import moments_cases as mc
import oracle_lib as ora
import sample_cases as sc
import test_gpu_agg_buckets as agg_tests
import trend_cases as tc
import modelardb_rs_amd as mdb

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
TILE = 64

_SHARED = {}


def _base():
    """One series of 1 500 points under a 1 % relative bound, compressed in chunks of 2..12 points: a few hundred short
    segments, one after the other in time."""
    if "base" not in _SHARED:
        timestamps, values = cc._series(1500, False, (41,), segment_length_range=(2, 12))
        cuts = np.concatenate([[0], np.cumsum(np.random.default_rng(42).integers(2, 13, 300))])
        cuts = np.append(cuts[cuts < len(timestamps) - 1], len(timestamps))
        eb = cases.error_bounds()["rel1"]
        _SHARED["base"] = mdb.SegmentBatch.concat([ora.try_compress_univariate_time_series(timestamps[a:b], values[0][a:b], eb)
                                                   for a, b in zip(cuts[:-1], cuts[1:])])
        assert 150 <= len(_SHARED["base"]) <= 1500
    return _SHARED["base"]


def _tiled():
    """The base series tiled to a little over 64^2 segments, as a comoments_cases.Field (the oracle's grid beside it)."""
    if "tiled" not in _SHARED:
        base = _base()
        copies = TILE * TILE // len(base) + 1
        _SHARED["tiled"] = cc.Field([base.take(np.tile(np.arange(len(base)), copies))])
        assert TILE * TILE < len(_SHARED["tiled"].batch) <= TILE * TILE + len(base)
    return _SHARED["tiled"]


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    for field in _SHARED.values():
        if isinstance(field, cc.Field):
            field.free()
    _SHARED.clear()


def _bucket_shapes(field):
    """(origin, width, n_buckets, what): one bucket over everything (pair order), two (the sort path)."""
    first, last = int(field.ts.min()), int(field.ts.max())
    return [(first, last - first + 1, 1, "one bucket, pair order"), (first, (last - first) // 2 + 1, 2, "two buckets, sorted")]


def _unsorted(field, origin, width):
    """Do the buckets of the segments' first rows ever go down in segment order?"""
    buckets = (field.batch.start_time.astype(np.int64) - origin) // width
    return bool((np.diff(buckets) < 0).any())


def test_the_shapes_are_what_the_tests_below_need():
    field = _tiled()
    (origin, width, _, _), (_, half, _, _) = _bucket_shapes(field)
    assert not _unsorted(field, origin, width) and _unsorted(field, origin, half)
    copies = len(field.batch) // len(_base())
    assert len(ic.field_intervals(field, None)) == len(field.ts) - copies   # (only the copies' seams are broken)


@pytest.mark.parametrize("method", [ic.LINEAR, ic.STEP], ids=["linear", "step"])
def test_integral_runs_through_every_level(hip, method):
    field = _tiled()
    for origin, width, n_buckets, what in _bucket_shapes(field):
        got = hip.integral_buckets(field.batch, origin, width, n_buckets, method=method)
        expected = ic.oracle(field, None, 1, origin, width, n_buckets, method)
        assert (expected["pieces"] > TILE * TILE // 2).all(), what
        ic.assert_cells(got, expected, f"integral {what}")
        on_device = hip.integral_buckets_dev(field.resident(hip), origin, width, n_buckets, method=method)
        assert on_device.tobytes() == got.tobytes(), what


def test_change_runs_through_every_level(hip):
    field = _tiled()
    for origin, width, n_buckets, what in _bucket_shapes(field):
        got = hip.change_buckets(field.batch, origin, width, n_buckets)
        expected = chc.oracle(field, None, 1, origin, width, n_buckets)
        assert (expected["count"] > TILE * TILE).all(), what
        chc.assert_cells(got, expected, f"change {what}")
        assert hip.change_buckets_dev(field.resident(hip), origin, width, n_buckets).tobytes() == got.tobytes(), what


def test_trend_runs_through_every_level(hip):
    field = _tiled()
    for origin, width, n_buckets, what in _bucket_shapes(field):
        got = hip.trend_buckets(field.batch, origin, width, n_buckets)
        expected = tc.oracle(field, None, 1, origin, width, n_buckets)
        assert (expected["count"] > TILE * TILE).all(), what
        cc.assert_cells(got, expected, f"trend {what}")
        assert hip.trend_buckets_dev(field.resident(hip), origin, width, n_buckets).tobytes() == got.tobytes(), what


def _sample_pairs():
    """A pair of the sampling operator is (segment, instant in the segment's extent), so one instant meets one segment
    of a series. Two neighbouring segments A, B of the base series, tiled: in every copy A's extent reaches over the
    link to B's first row. Returns the field and the time of A's last row and of B's first two."""
    if "sample" not in _SHARED:
        base = _base()
        a = len(base) // 2
        assert base.start_time[a + 1] - base.end_time[a] >= 2
        _SHARED["sample"] = cc.Field([base.take(np.tile([a, a + 1], TILE * TILE + 100))])
        _SHARED["sample_times"] = (int(base.end_time[a]), int(base.start_time[a + 1]))
    return _SHARED["sample"], _SHARED["sample_times"]


@pytest.mark.parametrize("method, name", sc.METHODS, ids=[name for _, name in sc.METHODS])
def test_sample_runs_through_every_level(hip, method, name):
    field, (a_last, b_first) = _sample_pairs()
    copies = len(field.batch) // 2
    assert copies > TILE * TILE
    inside_link = a_last + (b_first - a_last) // 2          # (strictly between A's last row and B's first)
    assert a_last < inside_link < b_first
    # One instant inside the link: one key, the pair of every copy's A, in pair order. Two instants, the second on B's
    # first row: the keys go 0 1 0 1 ... and are sorted.
    for origin, width, n, what in ((inside_link, INTERVAL, 1, "one instant, pair order"),
                                   (inside_link, b_first - inside_link, 2, "two instants, sorted")):
        got = hip.sample_at(field.batch, origin, width, n, method=method)
        expected = sc.oracle(field, None, 1, origin, width, n, method)
        if method != sc.EXACT:
            assert int(expected["count"][0, 0]) == copies, what   # (EXACT: no row on the instant, every partial empty)
        if n == 2:
            assert int(expected["count"][0, 1]) == copies, what
        sc.assert_cells(got, expected, f"sample {name} {what}")
        assert hip.sample_at_dev(field.resident(hip), origin, width, n, method=method).tobytes() == got.tobytes(), what


def _runs_around_a_tile_border():
    """384 segments in six groups of 63, 64, 65, 65, 64 and 63 - under one bucket a run of pairs each, ending at pair
    62 (before a border), 126, 191 (on one), 256 (the first pair behind one), 320 (as well) and 383 (on one)."""
    sizes = (63, 64, 65, 65, 64, 63)
    base = _base()
    assert len(base) >= 65
    batch = base.take(np.concatenate([np.arange(size) for size in sizes]))
    groups = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    ends = np.cumsum(sizes) - 1
    assert sorted(set(int(e) % TILE for e in ends)) == [0, 62, 63]
    return batch, groups, len(sizes)


def test_agg_runs_that_end_around_a_tile_border(hip):
    batch, groups, n_groups = _runs_around_a_tile_border()
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    got = hip.agg_buckets(batch, first, last - first + 1, 1, groups=groups, n_groups=n_groups)
    magnitudes = []
    expected = agg_tests._oracle_by_grid(batch, groups, n_groups, first, last - first + 1, 1, magnitudes=magnitudes)
    agg_tests._assert_cells(got, expected, "runs of 63, 64, 65 pairs", magnitudes[0])
    resident = hip.upload_segments(batch)
    on_device = hip.agg_buckets_dev(resident, first, last - first + 1, 1, groups=groups, n_groups=n_groups)
    resident.free()
    assert on_device.tobytes() == got.tobytes()


def test_moments_runs_that_end_around_a_tile_border(hip):
    batch, groups, n_groups = _runs_around_a_tile_border()
    first, last = int(batch.start_time.min()), int(batch.end_time.max())
    got = hip.moments_buckets(batch, first, last - first + 1, 1, groups=groups, n_groups=n_groups)
    mc.assert_cells(got, mc.oracle(batch, groups, n_groups, first, last - first + 1, 1), "runs of 63, 64, 65 pairs")
    resident = hip.upload_segments(batch)
    on_device = hip.moments_buckets_dev(resident, first, last - first + 1, 1, groups=groups, n_groups=n_groups)
    resident.free()
    assert on_device.tobytes() == got.tobytes()
