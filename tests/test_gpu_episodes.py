"""Episodes on segments (mdb_episodes, mdb_episodes_list, mdb_episodes_dev, mdb_episodes_count_dev) against the
reference's plan GridExec -> FilterExec -> WindowAggExec -> AggregateExec: the oracle's grid plus numpy
(tests/episodes_cases.py: totalOrder keys, the "continues" rule on the row arrays, np.fmin / np.fmax, math.fsum).
first_row, count, t_first, t_last, min, max, group, first_segment, n_rows and n_passing exactly; sum within 1e-5 of
the sum of magnitudes. Expected values never come from the library under test, except in the tests that say they are
consistency checks."""

import numpy as np
import pytest

import cases
import datagen
import episodes_cases as ec
import oracle_lib as ora
import modelardb_rs_amd as mdb

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = ec.I64_MIN, ec.I64_MAX


@pytest.fixture(scope="module")
def context():
    ctx = mdb.Context(0)
    yield ctx
    ctx.close()


def check(context, table, flt, groups=None, forms=("host",), **rule):
    """The forms named agree with the reference (and so with each other); returns the host form's result."""
    expected, magnitudes, n_rows, n_passing, _ = ec.reference(table, flt, groups, **rule)
    n_groups = None if groups is None else int(np.max(groups)) + 1 if len(groups) else 1
    results = {}
    if "host" in forms:
        results["host"] = context.episodes(table.batch, flt, groups, n_groups, **rule)
    if "dev" in forms:
        dev = context.upload_segments(table.batch)
        try:
            results["dev"] = context.episodes_dev(dev, flt, groups, n_groups, **rule)
        finally:
            dev.free()
    for name, (got, got_rows, got_passing) in results.items():
        assert (got_rows, got_passing) == (n_rows, n_passing), name
        ec.assert_episodes(got, expected, magnitudes)
    first = next(iter(results.values()))
    for other in results.values():
        assert other[0].tobytes() == first[0].tobytes()
    return first[0], expected


# ---- tables, predicates, time ranges ---------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1, 2])
def test_main_tables(context, which):
    table = ec.main_tables()[which]
    ids = np.concatenate([t.batch.model_type_id for t in ec.main_tables()])
    assert set(ids.tolist()) == {mdb.MDB_PMC_MEAN_ID, mdb.MDB_SWING_ID, mdb.MDB_MACAQUE_V_ID}
    for t_lo, t_hi in ec.time_ranges(table):
        for name, bounds in ec.predicates(table):
            flt = mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **bounds)
            for groups in (table.groups, None):
                got, expected = check(context, table, flt, groups, forms=("host", "dev") if name == "band" else ("host",))
                if name in ("none", "empty"):
                    assert len(got) == 0
    # always true over the whole axis: one episode per series, stitched across every segment
    got, _ = check(context, table, mdb.value_filter(), table.groups)
    assert len(got) == 4 and int(got["count"].sum()) == len(table.ts)
    assert np.array_equal(got["group"], np.arange(4))


def test_edge_cases(context):
    table = ec.edge_table()
    assert np.isnan(table.values).any() and np.isinf(table.values).any()
    for t_lo, t_hi in ec.time_ranges(table):
        for name, bounds in ec.predicates(table) + [("nan_up", {"lo": float("inf"), "lo_open": True}), ("zero", {"lo": 0.0}),
                                                    ("minus_zero", {"lo": -0.0}), ("le_minus_zero", {"hi": -0.0})]:
            for max_gap in (None, 100, 99):
                check(context, table, mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **bounds), None, max_gap=max_gap)
    # an episode of equal finite values has min == max == that value
    got, _ = check(context, table, mdb.value_filter(lo=5.0, hi=5.0))
    assert len(got) > 0 and np.all(got["min"] == 5.0) and np.all(got["max"] == 5.0)


# ---- stitching -------------------------------------------------------------------------------------------------------

def _stitch_table(middle):
    """A Swing segment whose tail passes v >= 5.5, the hand-built PMC-Mean segments `middle`, a Swing segment whose
    head passes."""
    up = (np.arange(10, dtype=np.int64) * 100, np.arange(1, 11, dtype=np.float32))
    down = (2000 + np.arange(10, dtype=np.int64) * 100, np.arange(10, 0, -1).astype(np.float32))
    first, last = (ora.try_compress_univariate_time_series(ts, v, cases.LOSSLESS) for ts, v in (up, down))
    return ec.Table(mdb.SegmentBatch.concat([first, mdb.SegmentBatch.from_rows(ec.pmc_rows(middle)), last]))


def test_stitching_across_segments(context):
    flt = mdb.value_filter(lo=5.5)
    table = _stitch_table([(1000, 20.0, 6)])
    assert list(table.batch.model_type_id) == [mdb.MDB_SWING_ID, mdb.MDB_PMC_MEAN_ID, mdb.MDB_SWING_ID]
    assert list(table.rows) == [10, 6, 10]
    got, _ = check(context, table, flt, forms=("host", "dev"))
    assert len(got) == 1 and got["first_row"][0] == 5 and got["count"][0] == 5 + 6 + 5 and got["first_segment"][0] == 0
    # a failing single point in the middle segment's place
    table = _stitch_table([(1000, 0.0, 1)])
    got, _ = check(context, table, flt, forms=("host", "dev"))
    assert len(got) == 2 and list(got["count"]) == [5, 5] and list(got["first_segment"]) == [0, 2]
    # a zero-row segment between: it lies beyond the time range, the episode goes on across it
    table = _stitch_table([(1000, 20.0, 6), (10**9, 0.0, 6)])
    got, _ = check(context, table, mdb.value_filter(lo=5.5, t_hi=10_000), forms=("host", "dev"))
    assert len(got) == 1 and got["count"][0] == 16
    got, _ = check(context, table, flt)
    assert len(got) == 2
    # an episode that ends exactly at a segment's last row, one that begins exactly at a segment's row 0
    table = ec.Table(mdb.SegmentBatch.from_rows(ec.pmc_rows([(0, 20.0, 4), (400, 0.0, 4), (800, 20.0, 4), (1200, 0.0, 1),
                                                             (1300, 20.0, 1), (1400, 20.0, 2)])))
    got, _ = check(context, table, flt, forms=("host", "dev"))
    assert list(got["first_row"]) == [0, 8, 13] and list(got["count"]) == [4, 4, 3]


# ---- per-point paths ---------------------------------------------------------------------------------------------------

def _per_point_table(irregular, run_end):
    """One series of 200 points whose rows 0 .. run_end pass (values above 50), row run_end + 1 fails, the rest pass."""
    rng = np.random.default_rng(5 + run_end)
    values = rng.uniform(100.0, 200.0, 200).astype(np.float32)
    values[run_end + 1] = 0.0
    values[150] = 1.0
    ts = np.cumsum(rng.integers(1, 40, 200)).astype(np.int64) if irregular else np.arange(200, dtype=np.int64) * 100
    if irregular:
        values[:] = np.where(values > 50, np.float32(150.0), values)  # PMC-Mean runs on irregular timestamps
    return ec.Table(ora.try_compress_univariate_time_series(ts, values, cases.LOSSLESS)), ts


@pytest.mark.parametrize("irregular", [False, True])
@pytest.mark.parametrize("run_end", [62, 63, 64, 65, 127, 128])
def test_per_point_segments(context, monkeypatch, irregular, run_end):
    table, ts = _per_point_table(irregular, run_end)
    flt = mdb.value_filter(lo=50.0)
    got, _ = check(context, table, flt, forms=("host", "dev"))
    assert got["count"][0] == run_end + 1
    if not irregular:
        assert mdb.MDB_MACAQUE_V_ID in table.batch.model_type_id and table.rows.max() > 128
    gaps = np.diff(ts)
    for max_gap in (int(gaps.min()), int(gaps.min()) - 1, int(gaps.max()), int(gaps.max()) - 1, 0):
        check(context, table, flt, max_gap=max_gap)
    # slices of the per-point segments: everything but `sum` byte for byte
    plain = context.episodes(table.batch, flt, max_gap=int(gaps.max()) - 1)
    monkeypatch.setenv("MDB_FILTER_SLICE_POINTS", "70")
    sliced = context.episodes(table.batch, flt, max_gap=int(gaps.max()) - 1)
    assert ec.same_but_sum(plain[0], sliced[0]) and plain[1:] == sliced[1:]


def test_long_irregular_segment_and_slices(context, monkeypatch):
    """Irregular timestamps under a constant value: one PMC-Mean segment of several hundred rows walked 64 at a time;
    with the slice size lowered the main table's per-point segments straddle many slices."""
    rng = np.random.default_rng(9)
    ts = np.cumsum(rng.integers(1, 30, 700)).astype(np.int64)
    table = ec.Table(ora.try_compress_univariate_time_series(ts, np.full(700, 7.0, dtype=np.float32), cases.LOSSLESS))
    assert table.rows.max() > 128
    for max_gap in (None, 29, 28, 15, 1, 0):
        check(context, table, mdb.value_filter(), max_gap=max_gap, forms=("host", "dev"))
    main = ec.main_tables()[1]
    flt = mdb.value_filter(lo=float(np.median(main.values)))
    plain = check(context, main, flt, main.groups, max_gap=150)[0]
    monkeypatch.setenv("MDB_FILTER_SLICE_POINTS", "1000")
    sliced = check(context, main, flt, main.groups, max_gap=150)[0]
    assert ec.same_but_sum(plain, sliced)


def test_equal_timestamps_with_max_gap_zero(context):
    ts = np.array([100, 100, 200, 200, 200, 300], dtype=np.int64)
    table = ec.Table(ora.try_compress_univariate_time_series(ts, np.arange(6, dtype=np.float32), cases.LOSSLESS))
    got, _ = check(context, table, mdb.value_filter(), max_gap=0, forms=("host", "dev"))
    assert list(got["count"]) == [2, 3, 1]


# ---- groups ------------------------------------------------------------------------------------------------------------

def test_groups_and_backward_steps(context):
    rows = ec.pmc_rows([(0, 5.0, 10), (1000, 5.0, 10)])
    table = ec.Table(mdb.SegmentBatch.from_rows(rows))
    assert len(check(context, table, mdb.value_filter(), None, forms=("host", "dev"))[0]) == 1
    # times go on increasing across the boundary but the groups differ
    got, _ = check(context, table, mdb.value_filter(), np.array([0, 1], dtype=np.uint32), forms=("host", "dev"))
    assert list(got["group"]) == [0, 1] and list(got["count"]) == [10, 10]
    # no groups, the second series starts earlier: the step backwards breaks the episode
    table = ec.Table(mdb.SegmentBatch.from_rows(ec.pmc_rows([(500, 5.0, 10), (0, 5.0, 10)])))
    assert list(check(context, table, mdb.value_filter(), None, forms=("host", "dev"))[0]["first_row"]) == [0, 10]
    # a bad group id on a row the time range does not reach is still an error
    for call in (lambda: context.episodes(table.batch, mdb.value_filter(t_lo=400), np.array([0, 7], dtype=np.uint32), 2),
                 lambda: _dev(context, table, mdb.value_filter(t_lo=400), np.array([0, 7], dtype=np.uint32), 2)):
        with pytest.raises(mdb.HipError, match="group id"):
            call()


def _dev(context, table, flt, groups=None, n_groups=None, **rule):
    dev = context.upload_segments(table.batch)
    try:
        return context.episodes_dev(dev, flt, groups, n_groups, **rule)
    finally:
        dev.free()


# ---- max_gap, min_count, min_duration ----------------------------------------------------------------------------------

def test_max_gap_on_regular_data(context):
    table = ec.main_tables()[1]
    series_ts = ec.main_series()[0][0]
    delta = int(series_ts[1] - series_ts[0])
    flt = mdb.value_filter(lo=float(np.median(table.values)), t_hi=int(series_ts[-1]))
    for max_gap in (0, delta - 1, delta, delta + 1, I64_MAX):
        got, expected = check(context, table, flt, table.groups, max_gap=max_gap, forms=("host", "dev"))
    _, _, _, n_passing, _ = ec.reference(table, flt, table.groups)
    got, _ = check(context, table, flt, table.groups, max_gap=delta - 1)
    assert len(got) == n_passing and np.all(got["count"] == 1)  # every passing row an episode of its own


def test_minimum_filters(context):
    table = ec.main_tables()[2]
    flt = mdb.value_filter(lo=float(np.median(table.values)))
    everything, _, _, n_passing, _ = ec.reference(table, flt, table.groups)
    some = everything[len(everything) // 2]
    count, duration = int(some["count"]), int(some["t_last"] - some["t_first"])
    for rule in ({"min_count": count}, {"min_count": count + 1}, {"min_duration": duration}, {"min_duration": duration + 1},
                 {"min_count": count, "min_duration": duration}, {"min_count": 1}):
        got, expected = check(context, table, flt, table.groups, forms=("host", "dev"), **rule)
        assert context.episodes(table.batch, flt, table.groups, **rule)[2] == n_passing
    assert len(check(context, table, flt, table.groups, min_count=count)[0]) > \
        len(check(context, table, flt, table.groups, min_count=count + 1)[0])


# ---- forms -------------------------------------------------------------------------------------------------------------

def test_forms_agree_byte_for_byte(context):
    table = ec.main_tables()[1]
    flt = mdb.value_filter(lo=float(np.median(table.values)))
    rule = {"max_gap": 1000}
    expected, magnitudes, n_rows, n_passing, _ = ec.reference(table, flt, table.groups, **rule)
    host = context.episodes(table.batch, flt, table.groups, **rule)
    ec.assert_episodes(host[0], expected, magnitudes)
    assert context.episodes(table.batch, flt, table.groups, **rule)[0].tobytes() == host[0].tobytes()  # two runs
    n = len(table.batch)
    inside = int(expected["first_segment"][np.argmax(expected["count"])]) + 1  # a cut inside the longest episode
    for cuts in ([0, inside, n], [0, n // 5, 2 * n // 5, inside, 4 * n // 5, n]):
        cuts = sorted(set(cuts))
        batches = [table.batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        groups = [table.groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        listed = context.episodes_list(batches, flt, groups, **rule)
        assert listed[0].tobytes() == host[0].tobytes() and listed[1:] == host[1:]
    dev = context.upload_segments(table.batch)
    groups_ptr = context.upload_array(table.groups)
    out = context.dev_alloc(64 * (len(expected) + 1))
    try:
        assert context.episodes_dev(dev, flt, table.groups, **rule)[0].tobytes() == host[0].tobytes()
        assert context.episodes_count_dev(dev, flt, groups_ptr, 4, **rule) == (len(expected), n_rows, n_passing)
        # cap == n succeeds; cap == n - 1 fails with out untouched
        marker = np.frombuffer(bytes([0xA5]) * (64 * (len(expected) + 1)), dtype=np.uint8)
        context.dev_free(out)
        out = context.upload_array(marker)
        with pytest.raises(mdb.HipError, match="too small"):
            context.episodes_into_dev(dev, flt, out, len(expected) - 1, groups_ptr, 4, **rule)
        assert context.download_array(out, marker.size, np.uint8).tobytes() == marker.tobytes()
        assert context.episodes_into_dev(dev, flt, out, len(expected), groups_ptr, 4, **rule) == (len(expected), n_rows, n_passing)
        written = context.download_array(out, len(expected) + 1, mdb.EPISODE_DTYPE)
        assert written[:-1].tobytes() == host[0].tobytes() and written[-1:].tobytes() == bytes([0xA5]) * 64
    finally:
        context.dev_free(out)
        context.dev_free(groups_ptr)
        dev.free()


def test_consistency_with_the_masks(context):
    """A consistency check: with the minimum filters off the union of the episodes is exactly the set bits of
    mdb_mask_filter_dev, the episodes are disjoint, and n_passing == n_set."""
    for table in (ec.main_tables()[0], ec.main_tables()[2], ec.edge_table()):
        dev = context.upload_segments(table.batch)
        try:
            for t_lo, t_hi in ec.time_ranges(table)[:2]:
                for _, bounds in ec.predicates(table)[3:]:
                    flt = mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **bounds)
                    words = max(mdb.mask_words(len(table.ts)), 1)
                    mask_ptr = context.dev_alloc(8 * words)
                    try:
                        n_rows, n_set = context.mask_filter_dev(dev, flt, mask_ptr, words)
                        bits = context.download_mask(mask_ptr, n_rows)
                    finally:
                        context.dev_free(mask_ptr)
                    episodes, rows, passing = context.episodes_dev(dev, flt, max_gap=50)
                    assert (rows, passing) == (n_rows, n_set)
                    covered = np.zeros(n_rows + 1, dtype=np.int64)
                    np.add.at(covered, episodes["first_row"].astype(np.int64), 1)
                    np.add.at(covered, (episodes["first_row"] + episodes["count"]).astype(np.int64), -1)
                    assert np.array_equal(np.cumsum(covered)[:-1], bits.astype(np.int64))
        finally:
            dev.free()


# ---- seeded random cases -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(8))
def test_random_cases(context, monkeypatch, seed):
    """Small seeded series under a random error bound, cut into a few series; random predicate, time range, groups,
    max_gap, minimum filters and slice size - every form against the reference."""
    rng = np.random.default_rng(1000 + seed)
    bounds = cases.error_bounds()
    eb = bounds[str(rng.choice(["lossless", "rel1", "abs5", "rel5"]))]
    parts, t0 = [], 0
    for _ in range(int(rng.integers(1, 5))):
        length = int(rng.integers(40, 700))
        ts, v = datagen.generate_univariate_time_series(length, (2, 90), bool(rng.integers(0, 2)), (1.0, 1.05),
                                                        (100.0, 200.0), int(rng.integers(1, 1 << 30)))
        parts.append(ora.try_compress_univariate_time_series(ts + t0, v, eb))
        t0 = int(ts[-1]) + int(rng.integers(-50_000, 3000))  # the next series may begin earlier
    table = ec.Table(mdb.SegmentBatch.concat(parts))
    table_groups = np.repeat(np.arange(len(parts), dtype=np.uint32), [len(p) for p in parts])
    predicates, ranges = ec.predicates(table), ec.time_ranges(table)
    steps = np.diff(table.ts)
    gaps = [None, 0, 1, int(np.median(steps)), int(np.median(steps)) - 1, int(steps.max()), 5000]
    for _ in range(12):
        t_lo, t_hi = ranges[int(rng.integers(0, 2))]
        flt = mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **predicates[int(rng.integers(3, len(predicates)))][1])
        rule = {"max_gap": gaps[int(rng.integers(0, len(gaps)))], "min_count": int(rng.choice([0, 1, 2, 7])),
                "min_duration": int(rng.choice([0, 0, 150, 4000]))}
        if rule["max_gap"] is not None and rule["max_gap"] < 0:
            rule["max_gap"] = 0
        if rng.integers(0, 2):
            monkeypatch.setenv("MDB_FILTER_SLICE_POINTS", str(int(rng.choice([1, 64, 100, 1000]))))
        else:
            monkeypatch.delenv("MDB_FILTER_SLICE_POINTS", raising=False)
        check(context, table, flt, table_groups if rng.integers(0, 2) else None, forms=("host", "dev"), **rule)


# ---- scan levels -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many_segments():
    """1024 * 65 + 3 PMC-Mean segments of 1 - 3 rows: more than one block of the stitch and more than one wave of
    block sums. Every value is 3.0, but every 1000th segment's is 1.0."""
    n = 1024 * 65 + 3
    counts = 1 + (np.arange(n) * 7 + 3) % 3
    starts = np.concatenate([[0], np.cumsum(counts[:-1] * 100)])
    values = np.where(np.arange(n) % 1000 == 999, 1.0, 3.0)
    return ec.Table(mdb.SegmentBatch.from_rows(ec.pmc_rows(zip(starts.tolist(), values.tolist(), counts.tolist()))))


def test_scan_levels(context, many_segments):
    table = many_segments
    n_rows = len(table.ts)
    dev = context.upload_segments(table.batch)
    try:
        got, rows, passing = context.episodes_dev(dev, mdb.value_filter())
        assert (rows, passing) == (n_rows, n_rows) and len(got) == 1
        one = got[0]
        assert one["first_row"] == 0 and one["count"] == n_rows and one["first_segment"] == 0
        assert one["sum"] == float(np.sum(table.values.astype(np.float64)))  # small integers: exact in any grouping
        assert one["min"] == 1.0 and one["max"] == 3.0 and one["t_last"] == int(table.ts[-1])
        flt = mdb.value_filter(lo=2.0)
        expected, magnitudes, _, n_passing, _ = ec.reference(table, flt)
        assert len(expected) == 67
        got, rows, passing = context.episodes_dev(dev, flt)
        assert (rows, passing) == (n_rows, n_passing)
        ec.assert_episodes(got, expected, magnitudes)
        assert np.array_equal(got["sum"], expected["sum"])
        assert context.episodes(table.batch, flt)[0].tobytes() == got.tobytes()
    finally:
        dev.free()
