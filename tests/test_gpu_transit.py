"""Transitions between value cells per date_bin bucket on segments (mdb_transit_buckets*): counts[group][bucket][from][to],
the linked pairs of rows by the cells of their two values, in the bucket of the later row. The tables are
tests/comoments_cases.py's and hand-made batches of a handful of segments; the reference (tests/transit_cases.py)
applies the linked rule to the oracle's grid row by row in Python integers.

Every comparison is assert_array_equal: the operator counts and there is no tolerance anywhere. Expected values never
come from the library under test, except in the tests that say they are consistency checks between operators."""

import ctypes

import numpy as np
import pytest

import cases
import comoments_cases as cc
import dwell_cases as dc
import hist_buckets_cases as hbc
import oracle_lib as ora
import transit_cases as tc
import modelardb_rs_amd as mdb

pytestmark = pytest.mark.gpu

INTERVAL = cc.INTERVAL
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
MAX_EDGES = mdb.MDB_HIST_MAX_EDGES
MAX_ROWS_UNDER_16_EDGES = 4_096   # (group, bucket) rows a request may have under 16 edges: 9.5 MB of counters


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()


def _span(field):
    return int(field.ts.min()), int(field.ts.max())


def _compress(timestamps, values, eb=cases.LOSSLESS):
    return ora.try_compress_univariate_time_series(np.asarray(timestamps, dtype=np.int64),
                                                   np.asarray(values, dtype=np.float32), eb)


def _is_regular(batch):
    return np.array([n == 0 or (batch.timestamps.value(i)[0] & 0x80) == 0 for i, n in enumerate(batch.timestamps.lengths())])


def _check(hip, field, edges, groups, n_groups, origin, width, n_buckets, context, max_gap=None):
    got = hip.transit_buckets(field.batch, edges, origin, width, n_buckets, groups=groups, max_gap=max_gap, n_groups=n_groups)
    expected = tc.oracle(field, edges, groups, n_groups, origin, width, n_buckets, max_gap)
    assert got.shape == (n_groups, n_buckets, len(edges) + 1, len(edges) + 1) and got.dtype == np.uint64
    np.testing.assert_array_equal(got, expected, err_msg=context)
    return got


def _below_diagonal(counts):
    """The sum of counts[..., from, to] over from > to."""
    n_cells = counts.shape[-1]
    return (counts * np.tril(np.ones((n_cells, n_cells), dtype=np.uint64), -1)).sum(axis=(-2, -1), dtype=np.uint64)


@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "one_group"])
@pytest.mark.parametrize("f", [0, 1, 2], ids=["lossless", "rel1", "abs5"])
def test_parity_with_the_rows_and_with_the_change_operator(hip, f, grouped):
    """All three model types, regular and irregular timestamps, segments far longer and far shorter than 64 rows;
    every bucket set of comoments_cases with its time range dropped, under 1, 3 and 16 edges through the data (16 where
    the request has at most 4 096 rows of matrices; 4 groups x 64 buckets through the data among them); every counter
    compared. Promise (a): the counters of a row sum to change_buckets' count for the same request; promise (f): those
    below the diagonal are at most its n_fall (consistency checks between two operators)."""
    field = cc.main_table()[f]
    groups, n_groups = (field.groups, 4) if grouped else (None, 1)
    lists = {n: dc.edges_through(field.values, n) for n in (1, 3, 16)}
    assert [len(edges) for edges in lists.values()] == [1, 3, 16]
    first, last = _span(field)
    through = ("64_buckets_unaligned", first - 777, (last - first + 777) // 64 + 13, 64, I64_MIN, I64_MAX)
    filled = off_diagonal = 0
    for name, origin, width, n_buckets, _, _ in cc.bucket_sets(first, last) + [through]:
        change = hip.change_buckets(field.batch, origin, width, n_buckets, groups=groups, n_groups=n_groups)
        for n_edges, edges in lists.items():
            if n_edges == 16 and n_groups * n_buckets > MAX_ROWS_UNDER_16_EDGES:
                continue
            got = _check(hip, field, edges, groups, n_groups, origin, width, n_buckets, f"field {f} {name} {n_edges} edge(s)")
            np.testing.assert_array_equal(got.sum(axis=(2, 3), dtype=np.uint64), change["count"], err_msg=f"{name} {n_edges}")
            assert (_below_diagonal(got) <= change["n_fall"]).all(), f"{name} {n_edges}"
            filled += int((got > 0).sum())
            off_diagonal += int(got.sum()) - int(np.trace(got, axis1=2, axis2=3).sum())
    assert filled > 10_000 and off_diagonal > 1_000


def test_six_rows_by_hand(hip):
    """6 rows, 2 edges, 3 buckets [50, 200), [200, 350), [350, 500): a pair whose earlier row lies in the previous
    bucket, one whose earlier row lies in front of the origin, and one whose later row lies behind the last bucket."""
    field = cc.Field([_compress([0, 100, 200, 300, 400, 500], [1.0, 5.0, 2.0, 2.0, 9.0, 1.0])])
    assert field.ts.tolist() == [0, 100, 200, 300, 400, 500]
    edges = np.array([1.5, 4.5], dtype=np.float32)   # cells of the rows: 0, 2, 1, 1, 2, 0
    got = _check(hip, field, edges, None, 1, 50, 150, 3, "by hand")
    assert got[0, 0].tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0]]   # 0 -> 100: the earlier row in front of the origin
    assert got[0, 1].tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 0]]   # 100 -> 200 (from the previous bucket) and 200 -> 300
    assert got[0, 2].tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0]]   # 300 -> 400; 400 -> 500 lies behind the last bucket
    up, down = mdb.transit_crossings(got)
    assert up[0].tolist() == [[1, 1], [0, 0], [0, 1]] and down[0].tolist() == [[0, 0], [0, 1], [0, 0]]
    # one more bucket takes the dropped pair, and nothing else changes
    more = _check(hip, field, edges, None, 1, 50, 150, 4, "one more bucket")
    assert more[0, 3].tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0]] and more[0, :3].tobytes() == got[0].tobytes()


def test_pmc_mean_segments(hip):
    """One segment of 200 equal rows under buckets of 7 intervals and of 1: only [c][c], equal to change_buckets'
    count (a consistency check) and to the reference; and a constant NaN segment."""
    timestamps = 1_000 + np.arange(200, dtype=np.int64) * INTERVAL
    for level in (42.0, np.nan):
        part = _compress(timestamps, np.full(200, level, dtype=np.float32))
        assert len(part) == 1 and part.model_type_id[0] == mdb.MDB_PMC_MEAN_ID and _is_regular(part).all()
        field = cc.Field([part])
        edges = np.array([10.0, 40.0, 50.0], dtype=np.float32)
        cell = 3 if level != level else 2
        for origin, width in ((1_000, 7 * INTERVAL), (1_000, INTERVAL), (970, 7 * INTERVAL), (1_001, INTERVAL),
                              (5_050, 250), (0, 100_000)):
            n_buckets = (int(timestamps[-1]) - origin) // width + 2
            got = _check(hip, field, edges, None, 1, origin, width, n_buckets, f"pmc {level} {origin} {width}")
            count = hip.change_buckets(field.batch, origin, width, n_buckets)["count"]
            np.testing.assert_array_equal(got[0, :, cell, cell], count[0])
            assert int(got.sum()) == int(got[0, :, cell, cell].sum()) == 199 - (origin > 1_000) * ((origin - 1_000) // INTERVAL)
        for max_gap in (INTERVAL - 1, INTERVAL):
            got = _check(hip, field, edges, None, 1, 1_000, 7 * INTERVAL, 30, f"pmc gap {max_gap}", max_gap=max_gap)
            assert int(got.sum()) == (199 if max_gap == INTERVAL else 0)


def test_a_pmc_mean_segment_that_is_all_residuals(hip):
    """The compressor writes no such segment, so one is cut by hand from a PMC-Mean segment on regular timestamps with
    a residual tail: the tail alone, its timestamps stream holding the tail's length, behind a one-row segment."""
    series = cc._series(600, False, (11, 12, 13), segment_length_range=(20, 120))
    source = cc.Field([_compress(series[0], series[1][2], cases.error_bounds()["abs5"])])
    batch, regular = source.batch, _is_regular(source.batch)
    tails = [i for i in range(len(batch)) if batch.model_type_id[i] == mdb.MDB_PMC_MEAN_ID and regular[i]
             and batch.residuals.lengths()[i] > 0 and 3 <= batch.residuals.value(i)[-1] < source.rows[i]]
    assert tails
    i = tails[0]
    n, r = int(source.rows[i]), int(batch.residuals.value(i)[-1])
    before = int(source.rows[:i].sum())
    timestamps, values = source.ts[before:before + n], source.values[before:before + n]
    row = batch.rows()[i]
    tail = mdb.SegmentBatch.from_rows([(row[0], int(timestamps[n - r]), int(timestamps[-1]), r.to_bytes(2, "big")) + row[4:]])
    lead = _compress([int(timestamps[n - r]) - INTERVAL], [values[0]])
    field = cc.Field([mdb.SegmentBatch.concat([lead, tail])])
    assert np.array_equal(field.ts[1:], timestamps[n - r:]) and field.values[1:].tobytes() == values[n - r:].tobytes()
    assert field.rows.tolist() == [1, r]
    first, last = _span(field)
    edges = dc.edges_through(field.values, 3) if len(np.unique(field.values)) > 1 else field.values[:1]
    for origin, width in ((first, INTERVAL), (first - 30, 70), (first + 1, 7), (first - 500, 1_300)):
        got = _check(hip, field, edges, None, 1, origin, width, (last - origin) // width + 2, f"all residuals {width}")
        assert int(got.sum()) == r   # (the lead's pair and the tail's own)
    # the source field, residual tails behind models of both kinds
    first, last = _span(source)
    _check(hip, source, dc.edges_through(source.values, 16), None, 1, first - 20, 370, (last - first) // 370 + 2, "tails")


def _ramp(n, first_value, step, t0=1_000):
    """A Swing segment of n rows on regular timestamps: an exact line under an absolute bound. The compressor stores
    runs of fewer than 10 rows as values, so a shorter one is a 64-row segment with its end moved by hand: the end time,
    the stored length and the far one of min_value / max_value."""
    rows = max(n, 64)
    timestamps = t0 + np.arange(rows, dtype=np.int64) * INTERVAL
    values = (first_value + step * np.arange(rows)).astype(np.float32)
    part = _compress(timestamps, values, cases.error_bounds()["abs5"])
    assert len(part) == 1 and part.model_type_id[0] == mdb.MDB_SWING_ID and _is_regular(part).all()
    if n < rows:
        row = part.rows()[0]
        low, high = sorted((float(values[0]), float(values[n - 1])))
        part = mdb.SegmentBatch.from_rows([(row[0], row[1], int(timestamps[n - 1]), bytes([n]), low, high) + row[6:]])
        _, rebuilt, per_segment, _ = ora.grid_batch(part)
        assert per_segment.tolist() == [n] and rebuilt.astype(np.float32).tobytes() == values[:n].tobytes()
    return part


def _row_walks(field):
    """The rows of `field` again as batches the kernel walks row by row: a lossless rebuild (no single Swing segment),
    and one segment per row, every pair a link across a seam."""
    walks = []
    lossless = cc.Field([_compress(field.ts, field.values)])
    if not (len(lossless.batch) == 1 and lossless.batch.model_type_id[0] == mdb.MDB_SWING_ID):
        walks.append(("lossless", lossless))
    if len(field.ts) <= 1_000:
        walks.append(("row by row", cc.Field([mdb.SegmentBatch.concat([_compress([t], [v]) for t, v in zip(field.ts, field.values)])])))
    for _, walk in walks:
        assert np.array_equal(walk.ts, field.ts) and walk.values.tobytes() == field.values.tobytes()
    return walks


@pytest.mark.parametrize("n", [2, 3, 64, 65, 1_000])
def test_swing_ramps(hip, n):
    """Ramps up and down that stay in one cell, cross one edge, cross an edge exactly on a bucket's first row and on its
    last, and jump two cells per row (steep); each closed-form case again under max_gap == the sampling interval (still
    linked) and on batches of the same rows that are walked row by row: the closed form and the walk agree."""
    step = 20.0   # (beyond what PMC-Mean holds under the bound, whatever n)
    for name, part in (("up", _ramp(n, 100.0, step)), ("down", _ramp(n, 100.0 + step * n, -step))):
        field = cc.Field([part])
        values, first, last = field.values, *_span(field)
        assert len(values) == n and (np.diff(values) != 0).all()
        low, high = float(values.min()), float(values.max())
        middle = values[n // 2]
        rows_per_bucket = 7 if n > 7 else 1
        width = rows_per_bucket * INTERVAL
        row_first = min(rows_per_bucket, n - 1)          # the first row of the second bucket
        row_last = min(2 * rows_per_bucket - 1, n - 1)   # the last row of the second bucket
        on_first, on_last = values[row_first], values[row_last]
        # a value ON an edge lies above it: a ramp up crosses on the pair that ends at the row, a ramp down on the pair
        # that begins at it - which the last row has none of
        edge_rows = {"one edge": n // 2, "on a first row": row_first, "on a last row": row_last}
        half = step / 2
        steep = np.arange(low - half / 2, high + half, half, dtype=np.float64).astype(np.float32)[:MAX_EDGES]
        edge_lists = {"one cell": np.array([low - 10.0, high + 10.0], dtype=np.float32),
                      "one edge": np.array([middle], dtype=np.float32),
                      "on a first row": np.array([on_first], dtype=np.float32),
                      "on a last row": np.array([on_last], dtype=np.float32),
                      "both": np.unique(np.array([on_first, on_last, middle], dtype=np.float32)),
                      "steep": np.unique(steep)}
        walks = _row_walks(field)
        for edge_name, edges in edge_lists.items():
            for origin, w in ((first, width), (first - 30, 250), (first - 10, last - first + 20)):
                n_buckets = (last - origin) // w + 2
                if n_buckets * (len(edges) + 1) ** 2 > 4_100_000:
                    continue
                context = f"{n} rows {name}, {edge_name}, width {w}"
                got = _check(hip, field, edges, None, 1, origin, w, n_buckets, context)
                assert int(got.sum()) == n - 1
                off = int(got.sum()) - int(np.trace(got, axis1=2, axis2=3).sum())
                if edge_name == "one cell":
                    assert off == 0
                elif edge_name == "steep":
                    assert off == n - 1 == int(np.trace(got, offset=2 if name == "up" else -2, axis1=2, axis2=3).sum())
                elif edge_name in edge_rows and w != 250:
                    assert off == (1 if name == "up" else int(edge_rows[edge_name] < n - 1))
                still = hip.transit_buckets(field.batch, edges, origin, w, n_buckets, max_gap=INTERVAL)
                assert still.tobytes() == got.tobytes(), context
                for walk_name, walk in walks:
                    walked = _check(hip, walk, edges, None, 1, origin, w, n_buckets, f"{context}, {walk_name}")
                    assert walked.tobytes() == got.tobytes(), f"{context}, {walk_name}"


def test_swing_ramps_under_the_longest_edge_list(hip):
    """1 000 rows up and down under 4 095 edges, most rows in a cell of their own: the closed form gives way to the walk
    point by point. One bucket: 134 MB of counters, compared through the non-zero ones."""
    for name, part in (("up", _ramp(1_000, 100.0, 20.0)), ("down", _ramp(1_000, 30_000.0, -20.0))):
        field = cc.Field([part])
        first, last = _span(field)
        edges = dc.edges_through(field.values, MAX_EDGES)
        assert len(edges) == MAX_EDGES
        got = hip.transit_buckets(field.batch, edges, first, last - first + 1, 1)
        expected = tc.oracle(field, edges, None, 1, first, last - first + 1, 1)
        assert np.array_equal(np.flatnonzero(got), np.flatnonzero(expected)), name
        np.testing.assert_array_equal(got.reshape(-1)[np.flatnonzero(expected)], expected.reshape(-1)[np.flatnonzero(expected)])
        assert int(got.sum()) == 999 and int(np.trace(got[0, 0])) < 250   # (crossed cells x search steps > rows)


def _tailed_segment():
    """A segment on regular timestamps with a residual tail, as a batch of one, with its rows."""
    series = cc._series(600, False, (11, 12, 13), segment_length_range=(20, 120))
    source = cc.Field([_compress(series[0], series[1][2], cases.error_bounds()["abs5"])])
    regular = _is_regular(source.batch)
    tails = [i for i in range(len(source.batch)) if regular[i] and source.batch.residuals.lengths()[i] > 0]
    assert tails
    i = tails[0]
    before, n = int(source.rows[:i].sum()), int(source.rows[i])
    return source.batch.slice(i, i + 1), source.ts[before:before + n], source.values[before:before + n]


def test_short_segments_and_the_pair_across_a_seam(hip):
    """Segments of one and two rows; and the pair across a seam - its from-cell the left segment's last value (a
    residual tail's included), its to-cell the right segment's first - with the right segment PMC-Mean, Swing, MacaqueV
    and on irregular timestamps. A bucket one microsecond wide at the right segment's first row holds that pair alone."""
    rng = np.random.default_rng(5)
    n = 300
    timestamps = 1_000 + np.cumsum(rng.integers(1, 400, n))
    values = rng.normal(100.0, 20.0, n).astype(np.float32)
    cuts = np.concatenate([[0], np.minimum(np.cumsum(rng.integers(1, 4, n)), n)])
    cuts = cuts[:int(np.argmax(cuts == n)) + 1]
    sizes = np.diff(cuts)
    assert (sizes == 1).sum() > 20 and (sizes == 2).sum() > 20
    tiny = cc.Field([_compress(timestamps[a:b], values[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(tiny.ts, timestamps)
    first, last = _span(tiny)
    edges = dc.edges_through(values, 3)
    for origin, width, n_buckets in ((first - 55, 170, (last - first) // 170 + 2), (first, last - first + 1, 1)):
        got = _check(hip, tiny, edges, None, 1, origin, width, n_buckets, f"tiny {width}")
        assert int(got.sum()) == n - 1
    tailed, tailed_ts, tailed_values = _tailed_segment()
    plain = _compress(1_000 + np.arange(5) * INTERVAL, np.full(5, 7.0, dtype=np.float32))
    lefts = {"pmc": (plain, 1_400, np.float32(7.0)), "tail": (tailed, int(tailed_ts[-1]), tailed_values[-1])}
    edges = np.unique(np.concatenate([[7.0], dc.edges_through(tailed_values, 3), [300.0, 400.0, 900.0]]).astype(np.float32))
    for left_name, (left, left_last, left_value) in lefts.items():
        t0 = left_last + 3 * INTERVAL
        regular_ts = t0 + np.arange(20, dtype=np.int64) * INTERVAL
        irregular_ts = t0 + np.cumsum(np.concatenate([[0], rng.integers(1, 300, 19)]))
        noise = (350.0 + rng.uniform(-30.0, 30.0, 20)).astype(np.float32)
        rights = {"pmc": (_compress(regular_ts, np.full(20, 950.0, dtype=np.float32)), mdb.MDB_PMC_MEAN_ID, True),
                  "swing": (_ramp(20, 320.0, 20.0, t0=t0), mdb.MDB_SWING_ID, True),
                  "macaque": (_compress(regular_ts, noise), mdb.MDB_MACAQUE_V_ID, True),
                  "irregular": (_compress(irregular_ts, noise), None, False)}
        for right_name, (right, model, regular) in rights.items():
            assert len(right) >= 1 and bool(_is_regular(right)[0]) == regular and model in (None, right.model_type_id[0])
            field = cc.Field([mdb.SegmentBatch.concat([left, right])])
            at = int(field.rows[:len(left)].sum())
            assert int(field.ts[at]) == t0 and int(field.ts[at - 1]) == left_last
            assert field.values[at - 1].tobytes() == np.float32(left_value).tobytes()
            first, last = _span(field)
            context = f"{left_name} | {right_name}"
            _check(hip, field, edges, None, 1, first - 20, 370, (last - first) // 370 + 2, context)
            seam = _check(hip, field, edges, None, 1, t0, 1, 1, context + ", the seam alone")
            cell_from = int(np.searchsorted(edges, field.values[at - 1], side="right"))
            cell_to = int(np.searchsorted(edges, field.values[at], side="right"))
            assert int(seam.sum()) == 1 and seam[0, 0, cell_from, cell_to] == 1 and cell_from != cell_to


def test_a_segment_without_rows_links_nothing_across_it(hip):
    """end_time < start_time under a stored length rebuilds to no row; the rows 200 and 500 are consecutive rows of the
    grid, so the expected counters are written out by hand."""
    left, right = _compress([100, 200], [1.0, 2.0]).rows(), _compress([500, 600], [2.0, 7.0]).rows()
    broken = mdb.SegmentBatch.from_rows(left + [(0, 400, 300, bytes([5]), 9.0, 9.0, b"", b"")] + right)
    timestamps, _, per_segment, _ = ora.grid_batch(broken)
    assert timestamps.tolist() == [100, 200, 500, 600] and per_segment.tolist()[len(left)] == 0
    edges = np.array([1.5], dtype=np.float32)
    got = hip.transit_buckets(broken, edges, 0, 1_000, 1)
    assert got[0, 0].tolist() == [[0, 1], [0, 1]]   # 1 -> 2 and 2 -> 7
    whole = cc.Field([mdb.SegmentBatch.from_rows(left + right)])   # without it the two are linked: 2 -> 2
    got = _check(hip, whole, edges, None, 1, 0, 1_000, 1, "no hole")
    assert got[0, 0].tolist() == [[0, 1], [0, 2]]


def test_the_gap_rule(hip):
    """max_gap of delta - 1 (nothing inside a regular segment), delta and None, and of the seam's gap - 1 and gap across
    the hole between two segments; equal timestamps are not linked."""
    source = cc.main_table()[0].parts[0]
    whole = cc.Field([source])
    hole_at = int(whole.rows[:len(source) // 2].sum())
    timestamps, values = whole.ts.copy(), whole.values
    timestamps[hole_at:] += 10 * INTERVAL + 3
    field = cc.Field([mdb.SegmentBatch.concat([_compress(timestamps[:hole_at], values[:hole_at]),
                                               _compress(timestamps[hole_at:], values[hole_at:])])])
    assert np.array_equal(field.ts, timestamps)
    seam = int(timestamps[hole_at] - timestamps[hole_at - 1])
    n = len(timestamps)
    first, last = _span(field)
    edges = dc.edges_through(values, 16)
    args = (None, 1, first - 30, 7 * INTERVAL, (last - first) // (7 * INTERVAL) + 2)
    linked = {0: 0, INTERVAL - 1: 0, INTERVAL: n - 2, seam - 1: n - 2, seam: n - 1, None: n - 1}
    for max_gap, total in linked.items():
        got = _check(hip, field, edges, *args, f"max_gap {max_gap}", max_gap=max_gap)
        assert int(got.sum()) == total, max_gap
    for f in (0, 1, 2):
        irregular = cc.Field([cc.main_table()[f].parts[1]])
        gaps = np.diff(irregular.ts)
        first, last = _span(irregular)
        for max_gap in (int(np.median(gaps)), int(gaps.max()) - 1):
            got = _check(hip, irregular, dc.edges_through(irregular.values, 16), None, 1, first - 9, 1_111,
                         (last - first) // 1_111 + 2, f"irregular {f} {max_gap}", max_gap=max_gap)
            assert int(got.sum()) == int((gaps <= max_gap).sum()) < len(gaps)
    edges = np.array([1.5, 4.5], dtype=np.float32)
    equal = cc.Field([_compress([500], [1.0]), _compress([500], [2.0]), _compress([600], [5.0])])
    assert equal.ts.tolist() == [500, 500, 600]
    got = _check(hip, equal, edges, None, 1, 0, 1_000, 1, "equal timestamps")
    assert got[0, 0].tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0]]   # 2 -> 5 alone


def test_seams_between_groups_and_series(hip):
    edges = np.array([1.5, 4.5], dtype=np.float32)
    # a step backwards across a seam links nothing; the rows inside the segments are linked
    backward = cc.Field([_compress([500, 600], [1.0, 2.0]), _compress([100, 250], [5.0, 7.0])])
    assert backward.ts.tolist() == [500, 600, 100, 250]
    got = _check(hip, backward, edges, None, 1, 0, 200, 4, "backward")
    assert int(got.sum()) == 2 and got[0, 3, 0, 1] == 1 and got[0, 1, 2, 2] == 1
    # a group change in mid-series: the pair across the cut is gone, every other one stays
    series = cc.Field([cc.main_table()[1].parts[0]])
    first, last = _span(series)
    cut = len(series.batch) // 2
    groups = (np.arange(len(series.batch)) >= cut).astype(np.uint32)
    at = int(series.rows[:cut].sum())
    fine = dc.edges_through(series.values, 16)
    got = _check(hip, series, fine, groups, 2, first, 50 * INTERVAL, (last - first) // (50 * INTERVAL) + 1, "group change")
    assert got.sum(axis=(1, 2, 3)).tolist() == [at - 1, len(series.ts) - at - 1]
    # a group per segment: only the pairs inside segments are left
    each = (np.arange(len(series.batch)) % 3).astype(np.uint32)
    got = _check(hip, series, fine, each, 3, first, 50 * INTERVAL, (last - first) // (50 * INTERVAL) + 1, "a group per segment")
    assert int(got.sum()) == int((series.rows - 1).sum())
    # the series of the main table as groups: no pair from one series to the next
    field = cc.main_table()[2]
    first, last = _span(field)
    got = _check(hip, field, fine[::5], field.groups, 4, first, 100_000, (last - first) // 100_000 + 1, "series")
    assert got.sum(axis=(1, 2, 3)).tolist() == (np.bincount(field.groups[field.segment]) - 1).tolist()


def test_values_that_are_not_finite_and_both_zeros(hip):
    """NaN of both signs, both infinities and both zeros with an edge at +0.0: each is placed by its totalOrder key;
    NaN -> finite and finite -> NaN pairs are counted like any other."""
    bits = np.array([0xFFC00000, 0x80000000, 0x00000000, 0xFF800000, 0x7F800000, 0x7FC00000, 0xFFC00001, 0x3F800000],
                    dtype=np.uint32)
    values = bits.view(np.float32)
    timestamps = np.array([0, 10, 30, 60, 100, 150, 210, 280], dtype=np.int64)
    field = cc.Field([_compress(timestamps, values)])
    assert field.values.view(np.uint32).tolist() == bits.tolist()
    zero = np.array([0.0], dtype=np.float32)
    got = _check(hip, field, zero, None, 1, 0, 1_000, 1, "an edge at +0.0")
    # cells: -NaN 0, -0.0 0, +0.0 1, -inf 0, +inf 1, +NaN 1, -NaN 0, 1.0 1
    assert got[0, 0].tolist() == [[1, 3], [2, 1]]
    around = np.array([-np.inf, -0.0, 0.0, np.inf], dtype=np.float32)
    got = _check(hip, field, around, None, 1, 5, 100, 3, "edges at both infinities and both zeros")
    # cells: -NaN 0, -0.0 2, +0.0 3, -inf 1, +inf 4, +NaN 4, -NaN 0, 1.0 3
    assert got[0].sum(axis=0).tolist() == [[0, 0, 1, 1, 0], [0, 0, 0, 0, 1], [0, 0, 0, 1, 0], [0, 1, 0, 0, 0], [1, 0, 0, 0, 1]]
    for edge_field in cc.edge_table():
        first, last = _span(edge_field)
        n_groups = len(edge_field.parts)
        finite = edge_field.values[np.isfinite(edge_field.values)]
        edges = np.unique(np.concatenate([zero, dc.edges_through(finite, 16)]))
        for origin, width in ((first, 1 << 40), (first - 17, (last - first) // 50 + 1)):
            n_buckets = (last - origin) // width + 1
            got = _check(hip, edge_field, edges, edge_field.groups, n_groups, origin, width, n_buckets, f"edge table {width}")
            count = hip.change_buckets(edge_field.batch, origin, width, n_buckets, groups=edge_field.groups, n_groups=n_groups)["count"]
            np.testing.assert_array_equal(got.sum(axis=(2, 3), dtype=np.uint64), count)


def test_the_forms_and_two_runs_agree_and_a_call_adds(hip):
    field = cc.main_table()[1]
    batch, groups = field.batch, field.groups
    first, last = _span(field)
    edges = dc.edges_through(field.values, 16)
    args = (edges, first - 40, 2_900, (last - first + 40) // 2_900 + 1)
    expected = tc.oracle(field, edges, groups, 4, *args[1:])
    host = hip.transit_buckets(batch, *args, groups=groups, n_groups=4)
    np.testing.assert_array_equal(host, expected)
    resident = field.resident(hip)
    dev = hip.transit_buckets_dev(resident, *args, groups=groups, n_groups=4)
    again = hip.transit_buckets_dev(resident, *args, groups=groups, n_groups=4)
    # the list cut inside series: pairs cross from one input to the next
    cuts = [0, 3, len(batch) // 3, len(batch) // 3 + 1, len(batch) - 2, len(batch)]
    listed = hip.transit_buckets_list([batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])], *args,
                                      groups=[groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])], n_groups=4)
    assert host.tobytes() == dev.tobytes() == again.tobytes() == listed.tobytes()
    # ... while separate calls over the same pieces lose the pairs across the cuts
    parts = [hip.transit_buckets(batch.slice(a, b), *args, groups=groups[a:b], n_groups=4) for a, b in zip(cuts[:-1], cuts[1:])]
    assert int(sum(int(part.sum()) for part in parts)) < int(host.sum())
    # a call adds into counters that are not zero, in every form
    rng = np.random.default_rng(3)
    start = rng.integers(0, 1 << 40, host.shape).astype(np.uint64)
    for call in (lambda counts: hip.transit_buckets(batch, *args, groups=groups, counts=counts),
                 lambda counts: hip.transit_buckets_dev(resident, *args, groups=groups, counts=counts),
                 lambda counts: hip.transit_buckets_list([batch], *args, groups=[groups], counts=counts)):
        counts = start.copy()
        assert call(counts) is counts
        np.testing.assert_array_equal(counts, start + expected)
    assert mdb.transit_merge(start.copy(), host).tobytes() == (start + expected).tobytes()
    # two calls over halves cut at a series boundary (no pair crosses it) equal one call
    cut = len(field.parts[0]) + len(field.parts[1])
    halves = (batch.slice(0, cut), batch.slice(cut, len(batch)))
    counts = hip.transit_buckets(halves[0], *args, groups=groups[:cut], n_groups=4)
    assert counts[:2].any() and not counts[2:].any()
    assert hip.transit_buckets(halves[1], *args, groups=groups[cut:], counts=counts).tobytes() == host.tobytes()


def _long_series():
    """One fully linked series of a few thousand rows on every kind of segment: series 0 of the main table, absolute 5."""
    field = cc.Field([cc.main_table()[2].parts[0]])
    assert (np.diff(field.ts) > 0).all() and 2_000 < len(field.ts) < 10_000
    return field


def test_finer_edges_finer_buckets_and_a_moved_origin(hip):
    """Promises (b) and (c): the blocks of adjacent cells added up give the matrix under the coarser edge list; buckets
    of width w summed in pairs equal buckets of width 2w; moving the origin by whole widths, with n_buckets moved
    along, gives the same numbers. Each side is also held to the reference."""
    field = _long_series()
    first, last = _span(field)
    fine = dc.edges_through(field.values, 15)
    coarse = fine[3::4]
    width = 1_700
    n_buckets = 2 * ((last - first + 40) // (2 * width) + 1)
    args = (None, 1, first - 40, width, n_buckets)
    by_fine = _check(hip, field, fine, *args, "fine")
    by_coarse = _check(hip, field, coarse, *args, "coarse")
    blocks = np.add.reduceat(np.add.reduceat(by_fine, [0, 4, 8, 12], axis=2), [0, 4, 8, 12], axis=3)
    np.testing.assert_array_equal(blocks, by_coarse)
    doubled = _check(hip, field, fine, None, 1, first - 40, 2 * width, n_buckets // 2, "width 2w")
    np.testing.assert_array_equal(by_fine[:, 0::2] + by_fine[:, 1::2], doubled)
    for shift in (3, -2):   # (origin - shift * width: `shift` more buckets in front, or fewer)
        moved = _check(hip, field, fine, None, 1, first - 40 - shift * width, width, n_buckets + shift, f"moved {shift}")
        if shift > 0:
            assert not moved[:, :shift].any()
            np.testing.assert_array_equal(moved[:, shift:], by_fine)
        else:
            np.testing.assert_array_equal(moved, by_fine[:, -shift:])


def test_arrivals_are_the_point_counts_and_crossings_telescope(hip):
    """Promise (d): the sum over `from` is hist_buckets' count of the bucket's rows minus the series' first row (a
    consistency check between two operators). Promise (e): over buckets that cover the run, the sum of up[e] - down[e]
    is (cell(last) > e) - (cell(first) > e)."""
    field = _long_series()
    first, last = _span(field)
    edges = dc.edges_through(field.values, 16)
    for origin, width in ((first, 1_700), (first - 123, 100_000), (first - 5, last - first + 10)):
        n_buckets = (last - origin) // width + 1
        got = _check(hip, field, edges, None, 1, origin, width, n_buckets, f"arrivals {width}")
        points = hip.hist_buckets(field.batch, edges, origin, width, n_buckets)
        np.testing.assert_array_equal(points, hbc.expected(field.batch, edges, (origin, width, n_buckets, None, None)))
        arrivals = got.sum(axis=2, dtype=np.uint64)
        cell_first = int(np.searchsorted(edges, field.values[0], side="right"))
        points[0, 0, cell_first] -= 1
        np.testing.assert_array_equal(arrivals, points)
        up, down = mdb.transit_crossings(got)
        reference_up, reference_down = tc.crossings(got)
        np.testing.assert_array_equal(up, reference_up)
        np.testing.assert_array_equal(down, reference_down)
        net = up.astype(np.int64).sum(axis=(0, 1)) - down.astype(np.int64).sum(axis=(0, 1))
        cell_last = int(np.searchsorted(edges, field.values[-1], side="right"))
        assert net.tolist() == [int(cell_last > e) - int(cell_first > e) for e in range(len(edges))]
        assert up.sum() > 0 and down.sum() > 0


def test_the_longest_edge_list_in_the_dev_form(hip):
    """4 095 edges, one group, one bucket, on a resident batch: 134 MB of counters and the kernel's whole table of edges.
    Compared through the non-zero counters."""
    field = cc.main_table()[0]
    first, last = _span(field)
    edges = dc.edges_through(field.values, MAX_EDGES)
    assert len(edges) == MAX_EDGES
    got = hip.transit_buckets_dev(field.resident(hip), edges, first, last - first + 1, 1)
    expected = tc.oracle(field, edges, None, 1, first, last - first + 1, 1)
    assert got.shape == (1, 1, MAX_EDGES + 1, MAX_EDGES + 1)
    hit = np.flatnonzero(expected)
    assert np.array_equal(np.flatnonzero(got), hit) and len(hit) > 500
    np.testing.assert_array_equal(got.reshape(-1)[hit], expected.reshape(-1)[hit])


def test_errors_on_the_device_leave_the_counters_untouched(hip):
    field = cc.main_table()[1]
    batch, groups = field.parts[0], np.arange(len(field.parts[0]), dtype=np.uint32) % 3
    rng = np.random.default_rng(9)
    edges = np.array([100.0, 150.0], dtype=np.float32)
    counts = np.frombuffer(rng.bytes(3 * 10 * 9 * 8), dtype=np.uint64).reshape(3, 10, 3, 3).copy()
    before = counts.copy()
    resident = hip.upload_segments(batch)
    data = counts.ctypes.data_as(ctypes.c_void_p)
    e = edges.ctypes.data_as(ctypes.c_void_p)
    seg = batch.as_c()
    # counters that do not fit the device: asked before `data` (a host pointer here) is touched
    large = hip._transit_request(0, 1000, 1 << 44, 3, None)
    for call in (lambda: hip.lib.mdb_transit_buckets(hip.handle, ctypes.byref(seg), None, ctypes.byref(large), e, 2, data),
                 lambda: hip.lib.mdb_transit_buckets_dev(hip.handle, ctypes.byref(resident.seg), None, ctypes.byref(large), e, 2, data)):
        assert call() == 1 and b"do not fit" in hip.lib.mdb_last_error(), hip.lib.mdb_last_error()
        assert counts.tobytes() == before.tobytes()
    # a group id out of range, on a row no bucket reaches
    bad = groups.copy()
    bad[-1] = 3
    assert int(batch.start_time[-1]) > 10 * 1000 and int(batch.start_time[0]) < 10 * 1000
    for call in (lambda: hip.transit_buckets(batch, edges, 0, 1000, 10, groups=bad, counts=counts, n_groups=3),
                 lambda: hip.transit_buckets_list([batch.slice(0, 5), batch.slice(5, len(batch))], edges, 0, 1000, 10,
                                                  groups=[bad[:5], bad[5:]], counts=counts, n_groups=3),
                 lambda: hip.transit_buckets_dev(resident, edges, 0, 1000, 10, groups=bad, counts=counts, n_groups=3)):
        with pytest.raises(mdb.HipError, match="group id"):
            call()
        assert counts.tobytes() == before.tobytes()
    resident.free()
    # a truncated values buffer on a reached segment: five points of MacaqueV values in five bytes
    pmc = lambda start, level: (0, start, start + 400, bytes([5]), level, level, b"", b"")
    truncated = mdb.SegmentBatch.from_rows([pmc(0, 1.5), (2, 500, 900, bytes([5]), 0.0, 0.0, bytes([1, 2, 3, 4, 0]), b""),
                                            pmc(1_000, 2.5)])
    one = np.frombuffer(rng.bytes(20 * 9 * 8), dtype=np.uint64).reshape(1, 20, 3, 3).copy()
    one_before = one.copy()
    truncated_resident = hip.upload_segments(truncated)
    for call in (lambda: hip.transit_buckets(truncated, edges, 0, 100, 20, counts=one),
                 lambda: hip.transit_buckets_dev(truncated_resident, edges, 0, 100, 20, counts=one)):
        with pytest.raises(mdb.HipError, match="Malformed segment"):
            call()
        assert one.tobytes() == one_before.tobytes()
    truncated_resident.free()
    # ... and on the neighbour whose first point is read, which no bucket reaches itself: the buckets end at 500
    neighbour = mdb.SegmentBatch.from_rows([pmc(0, 1.5), (2, 500, 900, bytes([5]), 0.0, 0.0, b"ab", b"")])
    neighbour_resident = hip.upload_segments(neighbour)
    five = one[:, :5].copy()
    for call in (lambda: hip.transit_buckets(neighbour, edges, 0, 100, 5, counts=five),
                 lambda: hip.transit_buckets_dev(neighbour_resident, edges, 0, 100, 5, counts=five)):
        with pytest.raises(mdb.HipError, match="Malformed segment"):
            call()
        assert five.tobytes() == one_before[:, :5].tobytes()
    neighbour_resident.free()
    # the same segments without the broken one are fine: the pair across the hole belongs to the bucket of 1 000
    whole = hip.transit_buckets(mdb.SegmentBatch.from_rows([pmc(0, 1.5), pmc(1_000, 2.5)]), edges, 0, 100, 20)
    assert whole[0, :, 0, 0].tolist() == [0, 1, 1, 1, 1] + [0] * 5 + [1, 1, 1, 1, 1] + [0] * 5 and int(whole.sum()) == 9


def test_nothing_to_do_succeeds_and_changes_nothing(hip):
    batch = cc.main_table()[1].parts[0]
    groups = np.arange(len(batch), dtype=np.uint32) % 3
    rng = np.random.default_rng(10)
    edges = np.array([100.0, 150.0], dtype=np.float32)
    counts = np.frombuffer(rng.bytes(3 * 10 * 9 * 8), dtype=np.uint64).reshape(3, 10, 3, 3).copy()
    before = counts.copy()
    resident = hip.upload_segments(batch)
    hip.transit_buckets(batch.slice(0, 0), edges, 0, 100, 10, counts=counts, n_groups=3)
    hip.transit_buckets_list([], edges, 0, 100, 10, counts=counts, n_groups=3)
    hip.transit_buckets_list([batch.slice(0, 0), batch.slice(3, 3)], edges, 0, 100, 10, counts=counts, n_groups=3)
    # buckets no row reaches
    hip.transit_buckets(batch, edges, int(batch.end_time.max()) + 1, 100, 10, groups=groups, counts=counts)
    hip.transit_buckets_dev(resident, edges, -10_000, 100, 10, groups=groups, counts=counts)
    assert counts.tobytes() == before.tobytes()
    none = np.zeros((3, 0, 3, 3), dtype=np.uint64)
    assert hip.transit_buckets(batch, edges, 0, 100, 0, groups=groups, counts=none).shape == (3, 0, 3, 3)
    assert hip.transit_buckets_dev(resident, edges, 0, 100, 0, groups=groups, counts=none).shape == (3, 0, 3, 3)
    resident.free()


def test_the_convenience_is_one_bucket_over_the_span(hip):
    field = cc.main_table()[0]
    first, last = _span(field)
    edges = dc.edges_through(field.values, 16)
    got = hip.transit(field.batch, edges, groups=field.groups, n_groups=4, max_gap=INTERVAL)
    assert got.shape == (4, 17, 17)
    np.testing.assert_array_equal(got, tc.oracle(field, edges, field.groups, 4, first, last - first + 1, 1, INTERVAL)[:, 0])
    assert not hip.transit(field.batch.slice(0, 0), edges, n_groups=2).any()
    assert hip.transit(field.batch.slice(0, 0), edges, n_groups=2).shape == (2, 17, 17)
