"""The plan a resident batch keeps for its grid calls without a time range never changes an answer.

The first mdb_grid_batch_dev without a range on a batch the library owns plans into allocations of the batch's own
(KeptGridPlan, csrc/mdb_grid.hip: descriptors, counts, offsets, the serial list, the tile map) and publishes them when
the call has ended without an error; every later call under the same switches launches the reconstruction kernels
only. The kernels are the ones every grid call runs, so the shapes here are chosen for what can go wrong in the kept
arrays: their sizing at tile boundaries, what they point at, who frees them, and which calls may use them.

Every output buffer is filled with POISON before every call - a call that launches nothing hands the poison back, not
the previous call's bytes - and every answer is compared, as SHA-256 of all the call returned, with the operator
ALONE: a fresh context, a fresh upload, one call (tests/test_gpu_resident_state.py's reference). The alone answers are
tied to the oracle once per batch.

Not asserted: that device memory is given back (test 6 of the tier's description). The library's device info has the
size of the HBM, not what is free of it, so a leak of a kept plan would not show through the binding.
"""

import functools
import threading

import numpy as np
import pytest

import cases
import oracle_lib as ora
import resident_orders as ro
import modelardb_rs_amd as mdb
from modelardb_rs_amd import api

pytestmark = pytest.mark.gpu

POISON = 0xA5
KEEP = "MDB_GRID_PLAN_KEEP"
PLANNING = ("k_grid_prepass_simple", "k_grid_prepass", "k_scan_blocks", "k_grid_offsets", "k_grid_ts_count")
TILE_POINTS = 4096


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    ro.apply_setting(monkeypatch, "unset")
    monkeypatch.delenv(KEEP, raising=False)


# ---- the batches ------------------------------------------------------------------------------------------------------

class Shape:
    """A batch with the oracle's grid of it."""

    def __init__(self, name, batch):
        self.name, self.batch = name, batch
        ts, val, rows = ora.grid_batch(batch)[:3]
        self.ts = np.ascontiguousarray(ts, dtype=np.int64)
        self.val = np.ascontiguousarray(val, dtype=np.float32)
        self.rows = np.ascontiguousarray(rows, dtype=np.uint32)
        self.n = len(self.ts)


def _steps_and_ramps(n_points, seed):
    """n_points values in runs that are constant or linear, 100 apart in time."""
    rng = np.random.default_rng(seed)
    values = []
    while len(values) < n_points:
        run = int(rng.integers(2, 400))
        if rng.integers(0, 2):
            values += [float(rng.integers(100, 200))] * run
        else:
            values += list(float(rng.integers(100, 200)) + 0.5 * np.arange(run))
    return np.arange(n_points, dtype=np.int64) * 100 + 1_000, np.asarray(values[:n_points], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def shape(name):
    if name == "corpus":
        return Shape(name, ro.corpus_a().batch)
    if name == "corpus_b":
        return Shape(name, ro.corpus_b().batch)
    if name == "simple":   # PMC-Mean and Swing segments with regular timestamps only
        timestamps, values = _steps_and_ramps(30_000, 5)
        batch = ora.try_compress_univariate_time_series(timestamps, values, cases.error_bounds()["rel5"])
        assert set(batch.model_type_id.tolist()) == {mdb.MDB_PMC_MEAN_ID, mdb.MDB_SWING_ID}
        assert not ro.irregular_rows(batch).any()
        assert len(batch) > 128
        return Shape(name, batch)
    if name.startswith("points_"):   # a hand-made batch of that many points: the tile map and offsets[n] at a tile's edge
        n_points = int(name.split("_")[1])
        timestamps, values = _steps_and_ramps(n_points, n_points)
        made = Shape(name, ora.try_compress_univariate_time_series(timestamps, values, cases.LOSSLESS))
        assert made.n == n_points
        return made
    if name == "one_segment":   # n = 1, more than one tile
        timestamps = np.arange(2 * TILE_POINTS + 5, dtype=np.int64) * 100 + 1_000
        made = Shape(name, ora.try_compress_univariate_time_series(timestamps, np.full(len(timestamps), 37.0, dtype=np.float32),
                                                                   cases.LOSSLESS))
        assert len(made.batch) == 1
        return made
    if name == "two_point_segments":
        # 3 000 segments of two points: a tile with more than 1 024 segments (the search in global memory) and more
        # than 128 descriptors; below 65 536 segments, so that the tile path runs and not the fused one.
        rows, begin = [], 1_000
        for k in range(3_000):
            part = ora.try_compress_univariate_time_series(np.array([begin, begin + 700], dtype=np.int64),
                                                           np.array([k % 89 + 1.0, k % 89 + 1.0 if k % 2 else k % 97 + 3.0], dtype=np.float32),
                                                           cases.LOSSLESS)   # (a constant pair, or two values)
            assert len(part) == 1
            rows += part.rows()
            begin += 2_000
        made = Shape(name, mdb.SegmentBatch.from_rows(rows))
        assert len(made.batch) == 3_000 and made.n == 6_000 and np.all(made.rows == 2)
        return made
    raise KeyError(name)


# ---- one call ---------------------------------------------------------------------------------------------------------

def _poisoned(context, n_bytes):
    return context.upload_array(np.full(max(n_bytes, 16), POISON, dtype=np.uint8))


def _is_poison(context, pointer, n_bytes):
    return bool(np.all(context.download_array(pointer, max(n_bytes, 16), np.uint8) == POISON))


def grid_once(context, resident, n, with_rows=False):
    """One mdb_grid_batch_dev into poisoned buffers of n points: (digest of all it returned, rows_per_segment or None)."""
    out_ts, out_val = _poisoned(context, 8 * n), _poisoned(context, 4 * n)
    out_rows = _poisoned(context, 4 * len(resident)) if with_rows else None
    try:
        produced, metrics = context.grid_batch_dev(resident, out_ts, out_val, n, out_rows)
        ts, val = context.download_array(out_ts, n, np.int64), context.download_array(out_val, n, np.float32)
        rows = context.download_array(out_rows, len(resident), np.uint32) if with_rows else None
        return ro.digest(produced, ts, val, metrics), rows
    finally:
        for pointer in (out_ts, out_val, out_rows):
            if pointer is not None:
                context.dev_free(pointer)


@functools.lru_cache(maxsize=None)
def alone(name, setting="unset"):
    """The grid of shape(name) alone under `setting`, tied to the oracle: timestamps, values and the count, bit for bit."""
    made = shape(name)
    with pytest.MonkeyPatch.context() as patch:
        ro.apply_setting(patch, setting)
        patch.delenv(KEEP, raising=False)
        context = api.Context(0)
        try:
            resident = context.upload_segments(made.batch)
            try:
                out_ts, out_val = _poisoned(context, 8 * made.n), _poisoned(context, 4 * made.n)
                try:
                    produced, metrics = context.grid_batch_dev(resident, out_ts, out_val, made.n)
                    ts = context.download_array(out_ts, made.n, np.int64)
                    val = context.download_array(out_val, made.n, np.float32)
                finally:
                    context.dev_free(out_ts)
                    context.dev_free(out_val)
            finally:
                resident.free()
        finally:
            context.close()
    assert produced == made.n and metrics["rows_created"] == made.n
    assert np.array_equal(ts, made.ts), f"{name} alone under {setting}: timestamps are not the oracle's"
    assert np.array_equal(val.view(np.uint32), made.val.view(np.uint32)), f"{name} alone under {setting}: values are not the oracle's"
    return ro.digest(produced, ts, val, metrics)


def _profiled(context, call):
    """call() with the library's profile on: (its result, the names of the kernels it launched)."""
    context.profile_enable(True)
    try:
        context.profile_reset()
        result = call()
        launched = {name for name, (launches, _) in context.profile().items() if launches > 0}
    finally:
        context.profile_enable(False)
    return result, launched


def _planning(launched):
    return sorted(name for name in launched if name in PLANNING or name.startswith("k_mv_index_"))


def _reconstructs(launched):
    return "k_grid_tiles" in launched or "k_grid_tiles_jumps" in launched


# ---- 1: repeats -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["corpus", "simple", "points_1", "points_4095", "points_4096", "points_4097", "points_12288",
                                  "one_segment", "two_point_segments"])
def test_repeated_grids_equal_the_grid_alone(name):
    made, expected = shape(name), alone(name)
    context = api.Context(0)
    try:
        resident = context.upload_segments(made.batch)
        try:
            for call in range(3):
                assert grid_once(context, resident, made.n)[0] == expected, f"{name}: call {call} answers otherwise than alone"
        finally:
            resident.free()
    finally:
        context.close()


# ---- 2: structure -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["corpus", "simple", "two_point_segments"])
def test_a_repeated_grid_launches_the_reconstruction_only(name, monkeypatch):
    made, expected = shape(name), alone(name)
    context = api.Context(0)
    try:
        for keep in (None, "0", "1"):   # not set: keep; 0: keep and use nothing; 1: a limit of one byte
            if keep is None:
                monkeypatch.delenv(KEEP, raising=False)
            else:
                monkeypatch.setenv(KEEP, keep)
            resident = context.upload_segments(made.batch)
            try:
                for call in range(3):
                    (got, _), launched = _profiled(context, lambda: grid_once(context, resident, made.n))
                    assert got == expected, f"{name}, {KEEP}={keep}: call {call} answers otherwise than alone"
                    assert _reconstructs(launched), (name, keep, call, sorted(launched))
                    if keep is None and call > 0:
                        assert _planning(launched) == [], (name, call, sorted(launched))
                    else:
                        assert {"k_scan_blocks", "k_grid_offsets"} <= launched, (name, keep, call, sorted(launched))
                        assert launched & {"k_grid_prepass_simple", "k_grid_prepass"}, (name, keep, call, sorted(launched))
            finally:
                resident.free()
    finally:
        context.close()


# ---- 3: rows and capacity -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["corpus", "two_point_segments"])
def test_rows_capacity_and_count_on_a_kept_plan(name):
    made, expected = shape(name), alone(name)
    context = api.Context(0)
    try:
        resident = context.upload_segments(made.batch)
        try:
            assert context.grid_count_dev(resident) == made.n
            assert grid_once(context, resident, made.n)[0] == expected
            assert context.grid_count_dev(resident) == made.n
            got, rows = grid_once(context, resident, made.n, with_rows=True)   # rows asked for on the second call only
            assert got == expected
            assert np.array_equal(rows, made.rows)
            # one point of capacity too few: today's error, before anything is written
            out_ts, out_val, out_rows = _poisoned(context, 8 * made.n), _poisoned(context, 4 * made.n), _poisoned(context, 4 * len(made.batch))
            try:
                with pytest.raises(mdb.HipError, match=f"Output buffers too small: {made.n} data points but capacity {made.n - 1}"):
                    context.grid_batch_dev(resident, out_ts, out_val, made.n - 1, out_rows)
                assert _is_poison(context, out_ts, 8 * made.n) and _is_poison(context, out_val, 4 * made.n)
                assert _is_poison(context, out_rows, 4 * len(made.batch))
            finally:
                for pointer in (out_ts, out_val, out_rows):
                    context.dev_free(pointer)
            got, rows = grid_once(context, resident, made.n, with_rows=True)
            assert got == expected and np.array_equal(rows, made.rows)
            assert context.grid_count_dev(resident) == made.n
        finally:
            resident.free()
    finally:
        context.close()


# ---- 4: scratch independence --------------------------------------------------------------------------------------------

def test_a_kept_plan_does_not_live_in_scratch():
    small, large = shape("simple"), shape("corpus")
    assert len(large.batch) > len(small.batch) and large.n > small.n
    context = api.Context(0)
    try:
        a, b = context.upload_segments(small.batch), context.upload_segments(large.batch)
        try:
            # a larger batch's call on the same context in between: the scratch slots grow, that is are freed and made anew
            assert grid_once(context, a, small.n)[0] == alone("simple")
            assert grid_once(context, b, large.n)[0] == alone("corpus")
            assert grid_once(context, a, small.n)[0] == alone("simple")
            assert grid_once(context, b, large.n)[0] == alone("corpus")
            # other operators of the same batch in between: a grid under a time range, aggregates
            corpus = ro.corpus_a()
            operators = dict(ro.OPERATORS)
            alone_range = _alone_operator("grid range")
            alone_aggregates = _alone_operator("all four")
            assert operators["grid range"](context, b, corpus) == alone_range
            assert operators["all four"](context, b, corpus) == alone_aggregates
            assert grid_once(context, b, large.n)[0] == alone("corpus")
            context.trim()   # (every scratch slot is given back)
            assert grid_once(context, b, large.n)[0] == alone("corpus")
            assert grid_once(context, a, small.n)[0] == alone("simple")
            assert operators["grid range"](context, b, corpus) == alone_range
        finally:
            a.free()
            b.free()
    finally:
        context.close()


@functools.lru_cache(maxsize=None)
def _alone_operator(operator):
    corpus = ro.corpus_a()
    context = api.Context(0)
    try:
        resident = context.upload_segments(corpus.batch)
        try:
            return dict(ro.OPERATORS)[operator](context, resident, corpus)
        finally:
            resident.free()
    finally:
        context.close()


# ---- 5: switches ------------------------------------------------------------------------------------------------------

def test_switches_between_grids(monkeypatch):
    # The schedules together put every setting directly before and directly after every other one (ro.switch_schedules).
    made = shape("corpus")
    context = api.Context(0)
    try:
        for schedule, settings in enumerate(ro.switch_schedules()):
            resident = context.upload_segments(made.batch)
            try:
                before = "nothing"
                for position, setting in enumerate(settings):
                    ro.apply_setting(monkeypatch, setting)
                    assert grid_once(context, resident, made.n)[0] == alone("corpus", setting), (
                        f"schedule {schedule}, call {position}: the grid under {setting}, directly after one under {before}, "
                        "answers otherwise than alone")
                    before = setting
            finally:
                resident.free()
    finally:
        context.close()


def test_a_plan_serves_the_switches_it_was_made_under_only(monkeypatch):
    made = shape("corpus")
    context = api.Context(0)
    try:
        resident = context.upload_segments(made.batch)
        try:
            ro.apply_setting(monkeypatch, "mv-from-8")
            assert grid_once(context, resident, made.n)[0] == alone("corpus", "mv-from-8")
            (got, _), launched = _profiled(context, lambda: grid_once(context, resident, made.n))
            assert got == alone("corpus", "mv-from-8") and _planning(launched) == [], sorted(launched)
            ro.apply_setting(monkeypatch, "unset")
            for call in range(2):   # not used, and not replaced: every call under other switches plans
                (got, _), launched = _profiled(context, lambda: grid_once(context, resident, made.n))
                assert got == alone("corpus")
                assert {"k_scan_blocks", "k_grid_offsets"} <= launched, (call, sorted(launched))
            ro.apply_setting(monkeypatch, "mv-from-8")
            (got, _), launched = _profiled(context, lambda: grid_once(context, resident, made.n))
            assert got == alone("corpus", "mv-from-8") and _planning(launched) == [], sorted(launched)
        finally:
            resident.free()
    finally:
        context.close()


# ---- 6: contexts and threads ------------------------------------------------------------------------------------------

def test_a_plan_made_by_one_context_serves_another():
    made, expected = shape("corpus"), alone("corpus")
    first, second = api.Context(0), api.Context(0)
    try:
        for builder, user in ((first, second), (second, first)):
            resident = builder.upload_segments(made.batch)
            try:
                assert grid_once(builder, resident, made.n)[0] == expected
                (got, _), launched = _profiled(user, lambda: grid_once(user, resident, made.n))
                assert got == expected and _planning(launched) == [] and _reconstructs(launched), sorted(launched)
                assert grid_once(builder, resident, made.n)[0] == expected
                assert grid_once(user, resident, made.n)[0] == expected
            finally:
                resident.free()
    finally:
        first.close()
        second.close()


def test_two_first_calls_at_once():
    made, expected = shape("corpus"), alone("corpus")
    origin = api.Context(0)
    try:
        for upload in range(3):
            resident = origin.upload_segments(made.batch)
            contexts = [origin.clone(), origin.clone()]
            barrier = threading.Barrier(2)
            records, errors = [[], []], [None, None]

            def work(k):
                try:
                    barrier.wait(timeout=60)   # released together: both make the batch's first call
                    for _ in range(3):
                        records[k].append(grid_once(contexts[k], resident, made.n)[0])
                except BaseException as error:   # (asserted in the main thread)
                    errors[k] = error

            threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(2)]
            for thread in threads:
                thread.start()
            for thread in threads:
                thread.join(timeout=120)
            if any(thread.is_alive() for thread in threads):
                pytest.fail(f"upload {upload}: a thread is still inside a call after 120 s", pytrace=False)
            try:
                assert errors == [None, None], (upload, errors)
                assert records == [[expected] * 3] * 2, f"upload {upload}: a call answers otherwise than alone"
                (got, _), launched = _profiled(origin, lambda: grid_once(origin, resident, made.n))
                assert got == expected and _planning(launched) == [], sorted(launched)
            finally:
                resident.free()
                for context in contexts:
                    context.close()
    finally:
        origin.close()


# ---- 7: lifetime ------------------------------------------------------------------------------------------------------

def test_a_freed_batch_takes_its_plan_with_it():
    a, b = shape("corpus"), shape("corpus_b")
    assert a.n == b.n and alone("corpus") != alone("corpus_b")
    context = api.Context(0)
    try:
        for made, name in ((a, "corpus"), (b, "corpus_b"), (a, "corpus")):
            resident = context.upload_segments(made.batch)   # (of the sizes of the one freed before it)
            try:
                for call in range(2):
                    assert grid_once(context, resident, made.n)[0] == alone(name), f"{name}, call {call}, after another batch was freed"
            finally:
                resident.free()
    finally:
        context.close()


# ---- 8: a malformed batch ---------------------------------------------------------------------------------------------

def test_a_malformed_batch_keeps_no_plan():
    healthy = shape("corpus")
    broken = ro.malformed(ro.corpus_a())
    n = healthy.n + 512   # (room for what the cut stream claims)

    def raised(context, resident):
        with pytest.raises(mdb.HipError) as caught:
            grid_once(context, resident, n)
        return str(caught.value)

    reference = api.Context(0)
    try:
        resident = reference.upload_segments(broken)
        try:
            message_alone = raised(reference, resident)
        finally:
            resident.free()
    finally:
        reference.close()
    context = api.Context(0)
    try:
        resident = context.upload_segments(broken)
        try:
            assert raised(context, resident) == message_alone
            message, launched = _profiled(context, lambda: raised(context, resident))
            assert message == message_alone
            assert {"k_scan_blocks"} <= launched, sorted(launched)   # (the second call plans again: nothing was kept)
            assert raised(context, resident) == message_alone
        finally:
            resident.free()
        # the same context on a healthy upload afterwards
        resident = context.upload_segments(healthy.batch)
        try:
            for call in range(2):
                assert grid_once(context, resident, healthy.n)[0] == alone("corpus")
        finally:
            resident.free()
    finally:
        context.close()
