"""What a resident batch remembers between calls never changes an answer.

A batch that stays on the device keeps what its calls found out about it - cursors into its MacaqueV streams, the walk
of its timestamp streams, per-segment counts and sums, what whole segments add up to under a range, chain offsets and
three failure flags (MvIndex, csrc/mdb_common.hpp) - built by whichever call comes first, on that call's stream, and
read by every later call from any context. One invariant over tests/resident_orders.py's table of operators: a call
answers with the same bits whatever was called on the batch before, by whom, on which stream and under which earlier
switches.

The reference is each operator ALONE: a fresh context, a fresh upload, one call, free and close - per switch setting
(`alone`). The existing suite ties that single call to the oracle; test_alone_answers_are_the_oracles does it once
more here for the grid, the aggregates, the histogram and every later operator (ro.LATER: M4, moments, histograms and
quantiles per bucket, comoments, binned, trend, integral, sample, change, episodes - each against its own test file's
reference), so that the tier cannot agree with itself on a wrong value. Everything else is equality of digests
(SHA-256 over the bytes of all a call returned): there is no tolerance below the anchoring test.

The operators that take two batches read `resident.partner`: every walker uploads the corpus's partner next to the
batch (ro.upload) and frees both (ro.release). comoments runs as (x = batch, y = partner), binned as (x = partner,
y = batch): the partner's kept state is made by those two calls alone, cold in a first walk and warm in a second.

Left out on purpose: a batch freed while a call is still inside it, more than one device, mdb_grid_submit's pipeline.
"""

import threading

import numpy as np
import pytest

import binned_cases as bc
import cases
import change_cases as chc
import comoments_cases as cc
import episodes_cases as ec
import integral_cases as ic
import oracle_lib as ora
import resident_orders as ro
import sample_cases as sc
import trend_cases as tc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import api
from hist_buckets_cases import expected as hist_buckets_oracle, expected_quantiles as quantile_buckets_oracle
from m4_cases import assert_cells as m4_cells, oracle as m4_oracle
from moments_cases import assert_cells as moments_cells, oracle as moments_oracle
from test_gpu_agg import _assert_state

pytestmark = pytest.mark.gpu

K = ro.K
ROWS = ro.williams(K)
NAMES = [name for name, _ in ro.OPERATORS]
RAISED = b"raised HipError"


def _call(run, context, resident, corpus, catch=False):
    try:
        return run(context, resident, corpus)
    except mdb.HipError:
        if not catch:
            raise
        return RAISED


def _alone(corpus, make_resident=None, catch=False):
    """Every operator's digest from a context and an upload of its own."""
    out = {}
    for name, run in ro.OPERATORS:
        context = api.Context(0)
        try:
            resident = ro.upload(context, corpus) if make_resident is None else make_resident(context)
            try:
                out[name] = _call(run, context, resident, corpus, catch)
            finally:
                ro.release(resident)
        finally:
            context.close()
    return out


class Alone:
    """The reference answers: of the corpus under every switch setting (computed when the module's first test asks),
    of corpus_b and of the malformed batch under the default setting (when their tests ask). Left unchanged."""

    def __init__(self):
        self.corpus, self.corpus_b = ro.corpus_a(), ro.corpus_b()
        ro.corpus_conditions(self.corpus)
        ro.corpus_conditions(self.corpus_b)
        self.by_setting = {}
        for setting in ro.SETTINGS:
            with pytest.MonkeyPatch.context() as patch:
                ro.apply_setting(patch, setting)
                self.by_setting[setting] = _alone(self.corpus)
        self._others = {}

    def of(self, setting="unset"):
        return self.by_setting[setting]

    def of_other(self, corpus, catch=False):
        if corpus.name not in self._others:
            with pytest.MonkeyPatch.context() as patch:
                ro.apply_setting(patch, "unset")
                self._others[corpus.name] = _alone(corpus, catch=catch)
        return self._others[corpus.name]


@pytest.fixture(scope="module")
def alone():
    return Alone()


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    ro.apply_setting(monkeypatch, "unset")


def _walk(context_of, resident, corpus, row, expected, what, catch=False, after_call=None):
    """The calls of `row` in order, call j by context_of(j); every digest is the expected one."""
    before = "nothing"
    for position, operator in enumerate(row):
        name, run = ro.OPERATORS[operator]
        got = _call(run, context_of(position), resident, corpus, catch)
        assert got == expected[name], (f"{what}: '{name}' at position {position} of row {row[0]}, directly after "
                                       f"'{before}', {'raised' if got == RAISED else 'answers otherwise than'} alone")
        before = name
        if after_call:
            after_call(position)


# ---- the reference itself -------------------------------------------------------------------------------------------

def _later_operators_are_their_references(context, corpus, expected):
    """Every operator of ro.LATER: the call its entry makes, on an upload of its own as `alone` makes it, its digest
    the one `alone` has, and what it returned held to the reference and the tolerance of the operator's own test file
    (counts, durations, M4 points, histogram counters, order statistics and episodes exact; the f64 members within the
    contract's tolerance; a cell with a non-finite input not finite, its count exact)."""
    def call(name):
        resident = ro.upload(context, corpus)
        try:
            result = ro.CALLS[name](context, resident, corpus)
        finally:
            ro.release(resident)
        assert ro.split_digest(*ro.MEMBERS[name](result)) == expected[name], name   # (the same call as the reference's)
        return result

    batch, partner, groups, n_groups = corpus.batch, corpus.partner, corpus.groups, ro.N_GROUPS
    buckets = corpus.buckets + corpus.cut_range                 # origin, width, number, t_lo, t_hi
    m4_cells(call("m4"), m4_oracle(batch, groups, n_groups, *buckets), "m4")
    moments_cells(call("moments"), moments_oracle(batch, groups, n_groups, *buckets), "moments")
    assert np.array_equal(call("hist buckets"), hist_buckets_oracle(batch, corpus.edges, buckets, groups, n_groups))
    lo, hi, n_points = call("quantile buckets")
    lo_bits, hi_bits, n_expected, filled = quantile_buckets_oracle(batch, buckets, ro.QUANTILES, groups, n_groups)
    assert np.array_equal(n_points, n_expected) and int(filled.sum()) >= 16
    assert np.array_equal(lo.view(np.uint32)[filled], lo_bits[filled]) and np.array_equal(hi.view(np.uint32)[filled], hi_bits[filled])
    assert np.isnan(lo[~filled]).all() and np.isnan(hi[~filled]).all()
    field, other = cc.Field([batch]), cc.Field([partner.batch])
    cc.assert_cells(call("comoments"), cc.oracle(field, other, groups, n_groups, *buckets), "comoments")
    bc.assert_cells(call("binned"), bc.oracle(other, field, partner.edges, partner.groups, n_groups, *buckets), "binned")
    trend, trend_expected = call("trend"), tc.oracle(field, groups, n_groups, *buckets)
    cc.assert_cells(trend, trend_expected, "trend")
    special = {"trend": tc.assert_x_side(trend, trend_expected, "trend")}
    runs = corpus.run_groups
    for name, spans, oracle, assert_cells, extra in (
            ("integral", corpus.spans, ic.oracle, ic.assert_cells, (ic.LINEAR, ro.LINK_GAP)),
            ("sample", corpus.sample_spans, sc.oracle, sc.assert_cells, (sc.LINEAR, ro.LINK_GAP)),
            ("sample step", corpus.sample_spans, sc.oracle, sc.assert_cells, (sc.STEP, None)),
            ("change", corpus.spans, chc.oracle, chc.assert_cells, (ro.LINK_GAP,))):
        special[name] = 0
        for k, (got, span) in enumerate(zip(call(name), spans)):
            special[name] += assert_cells(got, oracle(field, runs, n_groups, *span, *extra), f"{name}, span {k}")[1]
    assert all(count > 0 for count in special.values()), special   # (cells with a NaN or an infinity were among them)
    episodes, n_rows, n_passing = call("episodes")
    reference, magnitudes, rows, passing, _ = ec.reference(ec.Table(batch), corpus.band, groups=runs, max_gap=ro.EPISODE_GAP)
    assert (n_rows, n_passing) == (rows, passing) and len(reference) >= 64
    ec.assert_episodes(episodes, reference, magnitudes)


def test_alone_answers_are_the_oracles(hip, alone):
    corpus, expected = alone.corpus, alone.of()
    ts, val = ora.grid_batch(corpus.batch)[:2]
    ts, val = np.ascontiguousarray(ts, dtype=np.int64), np.ascontiguousarray(val, dtype=np.float32)
    assert np.array_equal(ts, corpus.timestamps)
    assert expected["grid"] == ro.digest(ts, val), "the grid alone is not the oracle's, bit for bit"
    context = api.Context(0)
    resident = context.upload_segments(corpus.batch)
    try:
        oracle = ora.agg_batch(corpus.batch, ro.ALL)
        for name, which in (("count", mdb.MDB_AGG_COUNT), ("min max", mdb.MDB_AGG_MIN | mdb.MDB_AGG_MAX), ("all four", ro.ALL)):
            state = context.agg_batch_dev(resident, which)
            assert ro.digest(state) == expected[name], name   # (the same call as the reference's)
            if which & mdb.MDB_AGG_COUNT:
                assert state.count == oracle.count == len(val)
            if which & mdb.MDB_AGG_MIN:
                assert np.float32(state.min).tobytes() == np.float32(oracle.min).tobytes()
                assert np.float32(state.max).tobytes() == np.float32(oracle.max).tobytes()
            if which == ro.ALL:
                _assert_state(state, oracle)   # SUM: test_gpu_agg.py's tolerance
        counts = context.hist_dev(resident, corpus.edges, corpus.groups, n_groups=ro.N_GROUPS)
        assert ro.digest(counts) == expected["hist"]
        assert int(counts.sum()) == len(val)
        segment = np.repeat(np.arange(len(corpus.batch)), ora.grid_batch(corpus.batch)[2].astype(np.int64))
        cells = np.searchsorted(ro._keys(corpus.edges), ro._keys(val), side="right")
        n_cells = len(corpus.edges) + 1
        by_numpy = np.bincount(corpus.groups.astype(np.int64)[segment] * n_cells + cells, minlength=ro.N_GROUPS * n_cells)
        assert np.array_equal(counts, by_numpy.astype(np.uint64).reshape(ro.N_GROUPS, n_cells))
        _later_operators_are_their_references(context, corpus, expected)
        # ... and of the plain series, whose SUM is a number
        plain = ro.corpus_plain()
        ro.plain_conditions(plain)
        plain_resident = context.upload_segments(plain.batch)
        try:
            state = context.agg_batch_dev(plain_resident, ro.ALL)
        finally:
            plain_resident.free()
        assert ro.digest(state) == alone.of_other(plain)["all four"]
        assert np.isfinite(state.sum)
        _assert_state(state, ora.agg_batch(plain.batch, ro.ALL))
    finally:
        ro.release(resident)
        context.close()
    # the settings move work between kernels, not answers: whatever has one answer in the oracle has one here
    for setting in ro.SETTINGS:
        for name in ("grid", "grid range", "count", "min max", "grid filter", "hist", "quantile", "download", "m4",
                     "hist buckets", "quantile buckets"):
            assert alone.of(setting)[name] == expected[name], (setting, name)
        # ... and of the later operators every count, duration, extreme and episode; their f64 sums and moments may
        # be rounded otherwise by another decoder, and are digested apart (ro.split_digest)
        for name in ro.CALLS:
            assert ro.exact_part(alone.of(setting)[name]) == ro.exact_part(expected[name]), (setting, name)


# ---- order ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", range(K))
def test_call_order(hip, alone, row):
    resident = ro.upload(hip, alone.corpus)
    try:
        _walk(lambda j: hip, resident, alone.corpus, ROWS[row], alone.of(), "every cache cold at first")
        _walk(lambda j: hip, resident, alone.corpus, ROWS[row], alone.of(), "every cache warm")
    finally:
        ro.release(resident)


@pytest.mark.parametrize("row", range(K))
def test_call_order_where_every_kept_sum_shows(hip, alone, row):
    # The corpus holds NaN and both infinities: its SUM over the whole batch is NaN whatever the kept per-segment sums
    # (MvIndex::agg_walk_sums) say. The same rows on the series without those values (ro.corpus_plain), where every
    # segment's sum shows in the bits of the total.
    plain = ro.corpus_plain()
    expected = alone.of_other(plain)
    resident = ro.upload(hip, plain)
    try:
        _walk(lambda j: hip, resident, plain, ROWS[row], expected, "plain values, every cache cold at first")
        _walk(lambda j: hip, resident, plain, ROWS[row], expected, "plain values, every cache warm")
    finally:
        ro.release(resident)


# ---- contexts and streams ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", range(K))
def test_contexts_and_streams(hip, alone, row):
    import torch
    resident = ro.upload(hip, alone.corpus)
    clones, stream = [], None
    try:
        clones = [hip.clone(), hip.clone(), hip.clone()]
        clones[1].set_scratch_limit(1 << 20)
        stream = torch.cuda.Stream()
        clones[2].set_stream(stream.cuda_stream)
        contexts = [hip] + clones

        def trim(position):
            if position % 4 == 3:
                hip.trim()

        # (no synchronisation between the calls: who reads a cache first is on another stream than its builder)
        _walk(lambda j: contexts[j % 4], resident, alone.corpus, ROWS[row], alone.of(),
              "call j by context j mod 4 (origin, clone, clone with a scratch limit, clone on a torch stream)", after_call=trim)
    finally:
        ro.release(resident)
        for clone in clones:
            clone.close()
        del stream


# ---- switches ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", range(ro.N_SCHEDULES))
def test_switches_between_calls(hip, alone, monkeypatch, schedule):
    settings = ro.switch_schedules()[schedule]
    operators = ROWS[schedule] + ROWS[(schedule + K // 2) % K]
    assert len(settings) == len(operators) == 2 * K
    resident = ro.upload(hip, alone.corpus)
    try:
        before = ("nothing", "unset")
        for position, (operator, setting) in enumerate(zip(operators, settings)):
            name, run = ro.OPERATORS[operator]
            ro.apply_setting(monkeypatch, setting)
            got = run(hip, resident, alone.corpus)
            assert got == alone.of(setting)[name], (f"schedule {schedule}, call {position}: '{name}' under {setting}, directly "
                                                    f"after '{before[0]}' under {before[1]}, answers otherwise than alone")
            before = (name, setting)
    finally:
        ro.release(resident)


# ---- threads ----------------------------------------------------------------------------------------------------------

def test_first_use_from_several_threads(hip, alone):
    corpus, expected = alone.corpus, alone.of()
    for upload in range(3):
        resident = ro.upload(hip, corpus)
        clones = [hip.clone() for _ in range(4)]
        rows = [(upload + quarter * K // 4) % K for quarter in range(4)]
        barrier = threading.Barrier(4)
        records = [[] for _ in range(4)]
        errors = [None] * 4

        def work(k):
            try:
                barrier.wait(timeout=60)   # released together: the first builders race
                for operator in ROWS[rows[k]]:
                    name, run = ro.OPERATORS[operator]
                    records[k].append((name, run(clones[k], resident, corpus)))
            except BaseException as error:   # (asserted in the main thread)
                errors[k] = error

        threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(4)]
        for thread in threads:
            thread.start()
        for thread in threads:
            thread.join(timeout=120)
        if any(thread.is_alive() for thread in threads):
            pytest.fail(f"upload {upload}: a thread is still inside a call after 120 s (rows {rows})", pytrace=False)
        try:
            assert errors == [None] * 4, (upload, rows, errors)
            for k in range(4):
                assert [name for name, _ in records[k]] == [NAMES[operator] for operator in ROWS[rows[k]]]
                for position, (name, got) in enumerate(records[k]):
                    assert got == expected[name], (f"upload {upload}, thread {k} on row {rows[k]}: '{name}' at position "
                                                   f"{position} answers otherwise than alone (the other threads: rows {rows})")
        finally:
            ro.release(resident)
            for clone in clones:
                clone.close()


# ---- a freed batch ----------------------------------------------------------------------------------------------------

def test_a_freed_batch_leaves_nothing_behind(hip, alone):
    a, b = alone.corpus, alone.corpus_b
    alone_a, alone_b = alone.of(), alone.of_other(b)
    # Other answers, so that a leftover would show. Both series hold NaN, -inf and +inf and as many points, so COUNT,
    # MIN, MAX and SUM over the WHOLE batch are one answer for both: n, -inf, +inf and NaN. Every other operator
    # returns values, or aggregates of a part of them, and must answer otherwise.
    for values in (a.values, b.values):
        assert np.isnan(values).any() and np.isneginf(values).any() and np.isposinf(values).any()
    assert len(a.values) == len(b.values)
    same = {name for name in NAMES if alone_a[name] == alone_b[name]}
    assert same <= {"count", "min max", "all four", "sum"}, sorted(same)

    def upload_warm_free(corpus, expected, row, what):
        resident = ro.upload(hip, corpus)
        try:
            _walk(lambda j: hip, resident, corpus, ROWS[row], expected, what)
        finally:
            ro.release(resident)

    upload_warm_free(a, alone_a, 1, "the corpus, first")
    upload_warm_free(b, alone_b, 6, "corpus_b after the corpus was freed")
    upload_warm_free(a, alone_a, 11, "the corpus after corpus_b was freed")
    # a batch born on the device (it registers through the fit): corpus_b's series, one chunk each
    timestamps, values, offsets = ro.series_b()
    inputs = [hip.upload_array(array) for array in (timestamps, values, offsets)]
    try:
        fitted = hip.compress_chunks_dev(inputs[0], inputs[1], inputs[2], len(offsets) - 1, cases.LOSSLESS)
        try:
            # (its partner: the corpus, the same series before the factor, uploaded)
            born = ro.Corpus("born on the device", fitted.download(), timestamps, values, partner=a)
            ro.attach_partner(hip, fitted, born)
            cold = {name: run(hip, fitted, born) for name, run in (ro.OPERATORS[operator] for operator in ROWS[4])}
            _walk(lambda j: hip, fitted, born, ROWS[9], cold, "the fitted batch, every cache warm, against its first answers")
        finally:
            ro.release(fitted)
    finally:
        for pointer in inputs:
            hip.dev_free(pointer)
    upload_warm_free(a, alone_a, 14, "the corpus after a batch born on the device was freed")


# ---- a malformed stream -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", [0, K // 4, K // 2, (3 * K) // 4])
def test_a_malformed_stream_fails_the_same_way_in_every_order(hip, alone, row):
    # The corpus and one MacaqueV row whose values payload is cut to half its bytes (the truncation
    # test_fuzzed_segments_never_hang_and_agree_with_the_oracle and tests/test_gpu_hist.py drive through the host and
    # the resident forms): the cursor index is built once, found unusable and kept that way, the pass that fills
    # range_acc fails once and is not tried again. An operator that raises alone raises in every position; one that
    # never looks at that stream - COUNT, MIN | MAX, the download, a time range in front of it - answers as alone.
    # Of the later operators the episodes alone decode it: their filter has no time range. The seven under cut_range
    # plan their rows and pairs from start_time and end_time, and the row lies behind t_hi; integral, sample and change
    # decode the segments whose extent meets a bucket, and their spans end inside the last long stream. The partner
    # holds the same row whole (ro.malformed_corpus): the pair operators find x and y lined up.
    healthy = alone.corpus
    broken = ro.malformed_corpus(healthy)
    expected = alone.of_other(broken, catch=True)
    raising = sorted(name for name in NAMES if expected[name] == RAISED)
    assert {"grid", "all four", "sum", "hist", "quantile", "episodes"} <= set(raising), raising
    answering = ("count", "min max", "download", "m4", "moments", "hist buckets", "quantile buckets", "comoments", "binned",
                 "trend", "integral", "sample", "sample step", "change")
    assert all(expected[name] != RAISED for name in answering), raising
    resident = ro.upload(hip, broken)
    try:
        _walk(lambda j: hip, resident, broken, ROWS[row], expected, "one malformed stream", catch=True)
    finally:
        ro.release(resident)
    # the same context on a healthy upload afterwards
    resident = ro.upload(hip, healthy)
    try:
        _walk(lambda j: hip, resident, healthy, ROWS[(row + 1) % K], alone.of(), "a healthy upload after the malformed one")
    finally:
        ro.release(resident)
