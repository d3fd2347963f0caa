"""tests/resident_orders.py held to its promises (no GPU): the design of the orders, what the corpora hold, what the
digest tells apart and what the switch schedules cover."""

import ctypes
import itertools

import numpy as np
import pytest

import oracle_lib as ora
import resident_orders as ro
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi


@pytest.mark.parametrize("k", sorted({14, 16, ro.K}))
def test_the_orders_are_a_williams_design(k):
    rows = ro.williams(k)
    assert len(rows) == k and all(sorted(row) == list(range(k)) for row in rows)
    assert sorted(row[0] for row in rows) == list(range(k))     # first exactly once
    assert sorted(row[-1] for row in rows) == list(range(k))    # last exactly once
    neighbours = [(row[j], row[j + 1]) for row in rows for j in range(k - 1)]
    assert len(neighbours) == k * (k - 1) == len(set(neighbours))  # every ordered pair exactly once
    assert set(neighbours) == {(a, b) for a in range(k) for b in range(k) if a != b}
    with pytest.raises(ValueError):
        ro.williams(k + 1)


def test_the_operator_table():
    names = [name for name, _ in ro.OPERATORS]
    assert len(set(names)) == len(names) == ro.K and ro.K % 2 == 0 and ro.K >= 14
    for needed in ("grid", "grid range", "count", "min max", "all four", "range cut", "range whole", "buckets", "filter",
                   "grid filter", "mask", "buckets filter", "hist", "quantile", "download"):
        assert needed in names
    # one entry per later resident entry point, sample_at_dev under two methods
    later = [name for name, _, _ in ro.LATER]
    assert later == ["m4", "moments", "hist buckets", "quantile buckets", "comoments", "binned", "trend", "integral",
                     "sample", "sample step", "change", "episodes"]
    assert names[-len(later):] == later and ro.K == 28
    assert set(ro.CALLS) == set(ro.MEMBERS) == set(later)


def test_the_rows_the_tests_name_are_distinct():
    # (tests/test_gpu_resident_state.py: the freed-batch test's rows, the malformed-stream test's, the threads')
    rows = ro.williams(ro.K)
    for numbers in ([1, 6, 11, 14, 4, 9], [0, ro.K // 4, ro.K // 2, (3 * ro.K) // 4],
                    *[[(upload + quarter * ro.K // 4) % ro.K for quarter in range(4)] for upload in range(3)]):
        assert len({tuple(rows[number]) for number in numbers}) == len(numbers) and max(numbers) < ro.K
    for schedule in range(ro.N_SCHEDULES):
        assert schedule != (schedule + ro.K // 2) % ro.K


@pytest.mark.parametrize("which", ["corpus_a", "corpus_b"])
def test_the_corpora_hold_what_the_tier_needs(which):
    corpus = getattr(ro, which)()
    ro.corpus_conditions(corpus)
    if which == "corpus_a":
        assert len(corpus.batch) == 468 and len(corpus.timestamps) == 110_679
        assert corpus.partner is ro.corpus_b() and ro.corpus_b().partner is corpus


def test_the_spans_lie_in_front_of_and_behind_the_gaps():
    corpus = ro.corpus_a()
    (front, width, n_front), (rear, _, n_rear) = corpus.spans
    gaps = np.flatnonzero(np.diff(corpus.timestamps) > 1 << 31)
    assert len(gaps) == 3
    assert front < corpus.timestamps[0] and corpus.timestamps[gaps[0]] < front + width * n_front < corpus.timestamps[gaps[0] + 1]
    # (the point behind the last gap ends a segment that begins in front of it: the rear span begins with the next)
    assert corpus.timestamps[gaps[-1] + 1] < rear < corpus.timestamps[gaps[-1] + 2]
    assert corpus.cut_range[1] < rear + width * n_rear <= corpus.cut_range[1] + width
    # what the conditions are for: each of them fails on a request that misses what it asks for
    only_front = ro.Corpus("front", corpus.batch, corpus.timestamps, corpus.values, partner=corpus.partner)
    only_front.spans = (corpus.spans[0], (rear, width, 64))
    with pytest.raises(AssertionError):
        ro.span_conditions(only_front)          # (no long stream under the buckets)
    ungrouped = ro.Corpus("neighbours apart", corpus.batch, corpus.timestamps, corpus.values, partner=corpus.partner)
    ungrouped.run_groups = corpus.groups
    with pytest.raises(AssertionError):
        ro.span_conditions(ungrouped)           # (no link between two segments)
    one_group = ro.Corpus("one group", corpus.batch, corpus.timestamps, corpus.values, partner=corpus.partner)
    one_group.run_groups = np.zeros(len(corpus.batch), dtype=np.uint32)
    with pytest.raises(AssertionError):
        ro.episode_conditions(one_group)        # (no passing row in the second group)
    with pytest.raises(AssertionError):
        ro.span_conditions(ro.corpus_plain())   # (no NaN, no infinity)
    ro.span_conditions(ro.corpus_plain(), non_finite=False)


def test_the_split_digest_compares_the_exact_members_apart():
    cells = mdb.fresh_moments_cells((2, 3))
    cells["count"] = np.arange(6).reshape(2, 3)
    cells["mean"] = 1.5
    whole = ro.split_digest(*ro.MEMBERS["moments"](cells))
    other = cells.copy()
    other["m2"][1, 2] = np.nextafter(0.0, 1.0)
    moved = ro.split_digest(*ro.MEMBERS["moments"](other))
    assert moved != whole and ro.exact_part(moved) == ro.exact_part(whole)
    other["count"][0, 0] += 1
    assert ro.exact_part(ro.split_digest(*ro.MEMBERS["moments"](other))) != ro.exact_part(whole)
    with pytest.raises(AssertionError):
        ro.MEMBERS["moments"](mdb.fresh_m4_cells((2, 3)))   # (every member is named, or the split fails)
    episodes = np.zeros(3, dtype=mdb.EPISODE_DTYPE)
    exact, rounded = ro.MEMBERS["episodes"]((episodes, 7, 3))
    assert ro.split_digest(exact, rounded) != ro.split_digest(*ro.MEMBERS["episodes"]((episodes, 7, 4)))


def test_the_plain_corpus_shows_every_kept_sum_in_its_total():
    plain, corpus = ro.corpus_plain(), ro.corpus_a()
    ro.plain_conditions(plain)
    assert np.isfinite(plain.values).all() and np.abs(plain.values).max() < ro.PLAIN_BELOW
    with np.errstate(invalid="ignore"):   # (why the corpus itself cannot serve: its SUM is NaN whatever a segment adds)
        assert np.isnan(corpus.values.astype(np.float64).sum())


def test_the_two_corpora_differ_in_their_answers_and_not_in_their_kind():
    a, b = ro.corpus_a(), ro.corpus_b()
    assert np.array_equal(a.timestamps, b.timestamps)
    finite = np.isfinite(a.values) & (a.values != 0)
    assert finite.sum() > 100_000 and not np.any(a.values[finite] == b.values[finite])
    assert ro.batch_digest(a.batch) != ro.batch_digest(b.batch)
    timestamps, values, offsets = ro.series_b()
    assert np.array_equal(timestamps, b.timestamps) and values.tobytes() == b.values.tobytes()
    assert offsets[0] == 0 and offsets[-1] == len(values) and np.all(np.diff(offsets.astype(np.int64)) > 0)


def test_the_malformed_batch_is_the_corpus_and_one_row():
    corpus = ro.corpus_a()
    batch = ro.malformed(corpus)
    assert len(batch) == len(corpus.batch) + 1 and batch.slice(0, len(corpus.batch)).identical(corpus.batch)
    last = batch.rows()[-1]
    same = [row for row in corpus.batch.rows() if row[3] == last[3] and row[6][: len(last[6])] == last[6]]
    assert last[0] == mdb.MDB_MACAQUE_V_ID and same and len(last[6]) == len(same[0][6]) // 2 > 12
    assert last[1] > corpus.batch.end_time[-1]
    # ... and its partner: corpus_b and the same row with its payload whole, so the pair lines up and has one fault
    broken = ro.malformed_corpus(corpus)
    assert broken.batch.identical(batch) and broken.spans == corpus.spans and broken.cut_range == corpus.cut_range
    other = broken.partner.batch
    assert len(other) == len(corpus.partner.batch) + 1 and other.slice(0, len(other) - 1).identical(corpus.partner.batch)
    whole = other.rows()[-1]
    assert whole[:6] == last[:6] and whole[7:] == last[7:] and whole[6] == same[0][6]
    timestamps = np.asarray(ora.grid_batch(other)[0])      # (whole: the oracle decodes it)
    assert 200 <= len(timestamps) - len(corpus.timestamps) <= 400
    assert timestamps[len(corpus.timestamps)] == last[1] and timestamps[-1] == last[2]
    # every request but the episodes' ends in front of the row
    assert max(corpus.cut_range[1], *[origin + width * n for origin, width, n in corpus.spans + corpus.sample_spans]) < corpus.batch.end_time[-1] < last[1]


def _flipped(array, bit):
    raw = bytearray(array.tobytes())
    raw[bit // 8] ^= 1 << (bit % 8)
    return np.frombuffer(bytes(raw), dtype=array.dtype).reshape(array.shape)


def test_the_digest_sees_every_bit():
    rng = np.random.default_rng(5)
    arrays = [rng.integers(-5, 5, 7).astype(np.int64), rng.uniform(-1, 1, 5).astype(np.float32),
              rng.integers(0, 9, (2, 3)).astype(np.uint64), mdb.fresh_agg_states((2, 2))]
    state = _abi.AggStateC.fresh()
    metrics = {"rows_created": 5, "regular_segments": 2}
    base = ro.digest(*arrays, state, metrics, 17, None)
    assert base == ro.digest(*[a.copy() for a in arrays], _abi.AggStateC.fresh(), dict(metrics), 17, None)
    for k, array in enumerate(arrays):
        for bit in range(array.nbytes * 8):   # a one-bit change of any returned array
            changed = list(arrays)
            changed[k] = _flipped(array, bit)
            assert ro.digest(*changed, state, metrics, 17, None) != base, (k, bit)
    for bit in range(ctypes.sizeof(state) * 8):
        other = _abi.AggStateC.fresh()
        raw = (ctypes.c_ubyte * ctypes.sizeof(other)).from_address(ctypes.addressof(other))
        raw[bit // 8] ^= 1 << (bit % 8)
        assert ro.digest(*arrays, other, metrics, 17, None) != base, bit
    assert ro.digest(*arrays, state, {"rows_created": 6, "regular_segments": 2}, 17, None) != base
    assert ro.digest(*arrays, state, metrics, 18, None) != base
    assert ro.digest(*arrays, state, metrics, 17) != base
    # a NaN's payload and sign, the sign of a zero
    quiet = np.array([0x7FC00000, 0], dtype=np.uint32).view(np.float32)
    for bits in ([0x7FC00001, 0], [0xFFC00000, 0], [0x7FA00000, 0], [0x7FC00000, 0x80000000]):
        other = np.array(bits, dtype=np.uint32).view(np.float32)
        assert ro.digest(quiet) != ro.digest(other)
    # the same bytes as another type or shape, or cut differently, are another answer
    assert ro.digest(np.zeros(4, dtype=np.int32)) != ro.digest(np.zeros(4, dtype=np.float32))
    assert ro.digest(np.zeros((2, 2), dtype=np.int32)) != ro.digest(np.zeros(4, dtype=np.int32))
    assert ro.digest(b"ab", b"c") != ro.digest(b"a", b"bc")
    assert ro.digest([b"ab"], [b"c"]) != ro.digest([b"ab", b"c"], [])
    with pytest.raises(TypeError):
        ro.digest(1.5)   # (bit patterns, not rounded floats)


def test_the_switch_schedules_put_every_setting_next_to_every_other():
    schedules = ro.switch_schedules()
    assert schedules == ro.switch_schedules.__wrapped__()      # seeded and fixed
    assert len(schedules) >= 6 and all(len(schedule) == 2 * ro.K for schedule in schedules)
    assert set(ro.SETTINGS) == set(itertools.chain(*schedules)) and "unset" in ro.SETTINGS
    switches = {setting[0] for setting in ro.SETTINGS.values() if setting}
    assert switches == set(ro.SWITCHES)
    values = sorted(int(setting[1]) for setting in ro.SETTINGS.values() if setting and setting[0] == "MDB_GRID_MV_MIN_VALUES")
    assert len(values) == 2 and 2 <= values[0] < 1024 < values[1]   # either side of MV_DEFAULT_MIN_VALUES
    neighbours = {(schedule[j], schedule[j + 1]) for schedule in schedules for j in range(len(schedule) - 1)}
    for before in ro.SETTINGS:
        for after in ro.SETTINGS:
            if before != after:
                assert (before, after) in neighbours, (before, after)
