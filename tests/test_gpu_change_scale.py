"""mdb_change_buckets* past 2^32 rows: PMC-Mean segments of 10^6 points each on regular timestamps, built column by
column (tests/scale_cases.py), in 2 groups with 8 buckets. Nothing rebuilds a row: the expected count and duration come
from closed forms in Python integers, the value members from the levels at the segment boundaries (small integers, so
every sum is exact). The call is O(segments): it is timed, and a path that loops over rows would need minutes."""

import time

import numpy as np
import pytest

import scale_cases as scale
import modelardb_rs_amd as mdb

pytestmark = pytest.mark.gpu

POINTS = 1_000_000
DELTA = 10
PER_GROUP = 2_150
BASE = 1_700_000_000_000_000   # epoch-scale microseconds
N_BUCKETS = 8


def test_pmc_mean_segments_past_2_to_the_32_rows(hip):
    rng = np.random.default_rng(20261020)
    n_segments = 2 * PER_GROUP
    assert n_segments * POINTS > 1 << 32
    levels = rng.integers(0, 200, n_segments).astype(np.float32)
    levels[5], levels[6] = 17.0, 17.0   # (a boundary without a step)
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

    expected = np.zeros((2, N_BUCKETS), dtype=mdb.CHANGE_CELL_DTYPE)
    for b in range(N_BUCKETS):
        lo, hi = origin + b * width, origin + (b + 1) * width - 1
        r_lo = max(1, -((BASE - lo) // DELTA))      # the first later row at or behind lo: ceil((lo - BASE) / DELTA)
        r_hi = min(rows - 1, (hi - BASE) // DELTA)
        count = max(0, r_hi - r_lo + 1)
        expected["count"][:, b] = count
        expected["duration"][:, b] = count * DELTA
    for g in range(2):
        level = levels[g * PER_GROUP:(g + 1) * PER_GROUP].astype(np.int64)
        for k in range(1, PER_GROUP):               # the pair that crosses into segment k
            b = (BASE + k * POINTS * DELTA - origin) // width
            d = int(level[k] - level[k - 1])
            cell = expected[g, b]
            if d > 0:
                cell["rise"] += d
                cell["max_rise"] = max(cell["max_rise"], d)
            elif d < 0:
                cell["n_fall"] += 1
                cell["fall"] += -d
                cell["reset_sum"] += int(level[k])
                cell["max_fall"] = max(cell["max_fall"], -d)
    assert int(expected["count"].sum()) == 2 * (rows - 1) and expected["n_fall"].sum() > 1_000

    resident = hip.upload_segments(batch)
    try:
        hip.change_buckets_dev(resident, origin, width, N_BUCKETS, groups=groups, n_groups=2)   # (warm: scratch)
        began = time.perf_counter()
        got = hip.change_buckets_dev(resident, origin, width, N_BUCKETS, groups=groups, n_groups=2)
        seconds = time.perf_counter() - began
    finally:
        resident.free()
    print(f"{2 * rows} rows in {n_segments} PMC-Mean segments, {N_BUCKETS} buckets x 2 groups: {seconds * 1e3:.2f} ms")
    for member in mdb.CHANGE_CELL_DTYPE.names:
        np.testing.assert_array_equal(got[member], expected[member], err_msg=member)
    assert hip.change_buckets(batch, origin, width, N_BUCKETS, groups=groups, n_groups=2).tobytes() == got.tobytes()
    np.testing.assert_array_equal(mdb.change_finish(got, mdb.MDB_CHANGE_NET).sum(axis=1),
                                  [float(levels[PER_GROUP - 1] - levels[0]), float(levels[-1] - levels[PER_GROUP])])
    assert seconds < 2.0, "the O(1) path of PMC-Mean rows is not taken"
