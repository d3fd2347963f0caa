"""mdb_dwell_buckets* past 2^32 rows: PMC-Mean segments of 10^6 points each on regular timestamps, built column by
column (tests/scale_cases.py), in 2 groups with 8 buckets and 16 edges. Nothing rebuilds a row: the expected
microseconds come from interval arithmetic in Python integers - a segment holds its level from its first row to the
first row of the next segment of its group (the link across the seam belongs to the left segment), the last segment of
a group to its own last row. The call is O(segments x buckets): it is timed, and a path that loops over rows would need
minutes."""

import bisect
import time

import numpy as np
import pytest

import hist_buckets_cases as hbc
import scale_cases as scale

pytestmark = pytest.mark.gpu

POINTS = 1_000_000
DELTA = 10
PER_GROUP = 2_150
BASE = 1_700_000_000_000_000   # epoch-scale microseconds
N_BUCKETS = 8


def test_pmc_mean_segments_past_2_to_the_32_rows(hip):
    rng = np.random.default_rng(20261021)
    n_segments = 2 * PER_GROUP
    assert n_segments * POINTS > 1 << 32
    levels = rng.integers(0, 200, n_segments).astype(np.float32)
    within = np.arange(n_segments) % PER_GROUP
    starts = BASE + within.astype(np.int64) * (POINTS * DELTA)
    lengths = np.full(n_segments, POINTS, dtype=np.int64)
    batch = scale.simple_batch(np.full(n_segments, scale.PMC), starts, lengths, np.full(n_segments, DELTA), levels, levels,
                               np.zeros(n_segments, dtype=bool))
    groups = (np.arange(n_segments) // PER_GROUP).astype(np.uint32)
    rows = PER_GROUP * POINTS                       # of one group
    origin = BASE - 12_345
    width = (rows * DELTA + 12_345) // N_BUCKETS + 3
    assert origin + N_BUCKETS * width > BASE + (rows - 1) * DELTA
    edges = (12.5 * np.arange(1, 17)).astype(np.float32)   # (levels are integers: none lies on an edge's float neighbour)
    edge_keys = hbc.keys_of(edges).tolist()

    expected = np.zeros((2, N_BUCKETS, len(edges) + 1), dtype=np.uint64)
    for i in range(n_segments):
        k = i % PER_GROUP
        t0 = BASE + k * POINTS * DELTA
        t1 = t0 + POINTS * DELTA if k + 1 < PER_GROUP else t0 + (POINTS - 1) * DELTA
        cell = bisect.bisect_right(edge_keys, int(hbc.keys_of(levels[i:i + 1])[0]))
        for b in range((t0 - origin) // width, N_BUCKETS):
            a, e = max(t0, origin + b * width), min(t1, origin + (b + 1) * width)
            if e <= a:
                break
            expected[i // PER_GROUP, b, cell] += e - a
    assert expected.sum(axis=(1, 2)).tolist() == [(rows - 1) * DELTA] * 2 and (expected > 0).sum() > 200

    resident = hip.upload_segments(batch)
    try:
        hip.dwell_buckets_dev(resident, edges, origin, width, N_BUCKETS, groups=groups, n_groups=2)   # (warm: scratch)
        began = time.perf_counter()
        got = hip.dwell_buckets_dev(resident, edges, origin, width, N_BUCKETS, groups=groups, n_groups=2)
        seconds = time.perf_counter() - began
    finally:
        resident.free()
    print(f"{2 * rows} rows in {n_segments} PMC-Mean segments, {N_BUCKETS} buckets x 2 groups x {len(edges) + 1} cells: "
          f"{seconds * 1e3:.2f} ms")
    np.testing.assert_array_equal(got, expected)
    assert hip.dwell_buckets(batch, edges, origin, width, N_BUCKETS, groups=groups, n_groups=2).tobytes() == got.tobytes()
    duration = hip.integral_buckets(batch, origin, width, N_BUCKETS, groups=groups, n_groups=2, method=1)["duration"]
    np.testing.assert_array_equal(got.sum(axis=2, dtype=np.uint64), duration)
    assert seconds < 2.0, "the O(1) path of PMC-Mean rows is not taken"
