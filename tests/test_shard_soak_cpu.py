"""The plans and composed references of the shard soak (tests/shard_soak.py), held to their promises without a GPU over
the default indices 0 to 39: plan() is a pure function of its index; the shards of a plan put end to end are the batch;
under `seams` every composed reference equals the whole-case one exactly, which is what lets the GPU tier ask for the
bytes of the one call; under `anywhere` a severed link takes exactly its clipped microseconds out of the composed
durations; the plans hold what the soak exists for (the census floors); and the host folds the GPU tier uses exist and
refuse arrays of two sizes."""

import collections

import numpy as np
import pytest

import linked_soak as ls
import query_soak as qs
import sample_cases as sc
import shard_soak as ss
import modelardb_rs_amd as mdb

N_INDICES = 40
# What the plans of the indices 0 .. 39 must hold at least: conditions on the generator, counted from plan() alone.
FLOORS = {
    "kept cases": N_INDICES // 2,
    "cases with a forward same-group link over a segment boundary": 20,
    "forward same-group links over a segment boundary": 164,
    "cases whose anywhere plan severs a link": 20,
    "cases whose seams plan has a cut between groups": 13,
    "plans with an empty shard": 25,
    "shards that begin or end with a single-point segment": 50,
    "shards without a row of some group": 60,
    "series-order cases cut by series_range": 5,
    "series-order cases with more ranks than series": 4,
    "ranks without a series": 6,
    "cases whose anywhere plan cuts beside a single-point tail segment": 6,
    "cases with a sample request through a row that holds -0.0": 4,
    "sample cells whose one contribution is a row that holds -0.0": 4,
    "trend requests whose x stays below 2^53 (kept)": 120,
}


@pytest.fixture(scope="module")
def plans():
    out = {}
    for index in range(N_INDICES):
        planned = ss.plan(index)
        assert (planned is None) == (ls.draw(index) is None)   # (cases that draw leaves out stay left out; nothing else)
        if planned is not None:
            out[index] = planned
    yield out
    qs.forget_grids()


def test_a_plan_is_a_pure_function_of_its_index(plans):
    for index in list(plans)[:8]:
        assert ss.plan_bytes(ss.plan(index)) == ss.plan_bytes(plans[index]), index
    first, second = list(plans)[:2]
    assert ss.plan_bytes(plans[first]) != ss.plan_bytes(plans[second])


def test_the_shards_of_a_plan_are_the_batch(plans):
    for index, planned in plans.items():
        drawn = planned.drawn
        for one in planned.plans.values():
            for cuts in (one.cuts, one.episode_cuts):
                assert 2 <= len(cuts) + 1 <= 6 and cuts == sorted(cuts), (index, one.name)
                batches, groups = ss.shards(planned, cuts)
                assert sum(len(batch) for batch in batches) == len(drawn.batch)
                assert mdb.SegmentBatch.concat(batches).rows() == drawn.batch.rows(), (index, one.name)
                if drawn.groups is None:
                    assert groups is None
                else:
                    assert np.array_equal(np.concatenate(groups), drawn.groups), (index, one.name)
                    assert [len(g) for g in groups] == [len(batch) for batch in batches]
                # the rows of the shards are the rows of the case, in order
                ranges = ss._row_ranges(planned, cuts)
                assert ranges[0][0] == 0 and ranges[-1][1] == len(drawn.timestamps)
                assert all(a[1] == b[0] for a, b in zip(ranges[:-1], ranges[1:]))


def test_seams_cut_where_no_link_crosses(plans):
    """The rule itself, from the rows either side of every cut."""
    for index, planned in plans.items():
        drawn, one = planned.drawn, planned.plans["seams"]
        t, g = drawn.timestamps, drawn.row_groups
        for cut in one.cuts:
            if 0 < cut < len(drawn.batch):
                q = int(planned.starts[cut])
                assert g[q] != g[q - 1] or t[q] <= t[q - 1], (index, cut)
        assert not one.severed
        if one.world is not None:   # the rank blocks: every cut is the first segment of a series, or the end
            assert not drawn.permuted and drawn.grouping == "series"
            n_series = len(drawn.kinds)
            firsts = [int(np.flatnonzero(drawn.series_of_segment == k)[0]) for k in range(n_series)] + [len(drawn.batch)]
            assert len(one.cuts) == one.world - 1 and all(cut in firsts for cut in one.cuts), (index, one.cuts)


def test_under_seams_every_composed_reference_is_the_whole_one(plans):
    compared = collections.Counter()
    for index, planned in plans.items():
        drawn, one = planned.drawn, planned.plans["seams"]
        for request in drawn.requests:
            for method, _ in ls.INTEGRAL_METHODS:
                assert ss.same(ss.composed_integral(planned, one, request, method),
                               ls.reference_integral(drawn, request, method)), (index, ls.describe(request))
            assert ss.same(ss.composed_change(planned, one, request), ls.reference_change(drawn, request)), index
            assert ss.same(ss.composed_dwell(planned, one, request), ss.whole_dwell(planned, request)), index
            compared["requests"] += 1
        for request in planned.sample_requests:
            for method, _ in ls.SAMPLE_METHODS:
                composed, whole = ss.composed_sample(planned, one, request, method), ls.reference_sample(drawn, request, method)
                assert ss.same(composed, whole), (index, ls.describe(request), method)   # (the Fractions by value)
                compared["sample cells"] += int((whole["count"] > 0).sum())
        for rule in drawn.episodes:
            composed, whole = ss.composed_episodes(planned, one, rule), ls.reference_episodes(drawn, rule)[:4]
            assert len(composed[0]) == len(whole[0]), (index, vars(rule))
            for member in whole[0].dtype.names:
                assert composed[0][member].tobytes() == whole[0][member].tobytes(), (index, member)
            assert ss.same(composed, whole), index
            compared["episodes"] += len(whole[0])
    print(dict(compared))
    assert compared["requests"] > 100 and compared["sample cells"] > 10_000 and compared["episodes"] > 1000


def test_a_severed_link_takes_its_microseconds_out_of_the_composed_durations(plans):
    cases = differing = 0
    for index, planned in plans.items():
        drawn, one = planned.drawn, planned.plans["anywhere"]
        if not one.severed:
            continue
        cases += 1
        differs = False
        for request in drawn.requests:
            whole = ls.reference_integral(drawn, request, ls.INTEGRAL_METHODS[0][0])
            composed = ss.composed_integral(planned, one, request, ls.INTEGRAL_METHODS[0][0])
            lost = ss.severed_microseconds(planned, one, request, "integral")
            assert [a - b for a, b in zip(ss.duration_per_group(whole["duration"]),
                                          ss.duration_per_group(composed["duration"]))] == lost, (index, ls.describe(request))
            if sum(lost):
                assert not ss.same(composed["duration"], whole["duration"])
                differs = True
            whole, composed = ls.reference_change(drawn, request), ss.composed_change(planned, one, request)
            lost = ss.severed_microseconds(planned, one, request, "change")
            assert [(a - b) % (1 << 64) for a, b in zip(ss.duration_per_group(whole["duration"]),
                                                        ss.duration_per_group(composed["duration"]))] == \
                [x % (1 << 64) for x in lost], (index, ls.describe(request))
        differing += differs
    print(f"{cases} cases with a severed link, the composed integral duration differs from the whole one in {differing}")
    # (a case loses nothing only where the max_gap or the window of every one of its requests excludes the severed links)
    assert cases >= FLOORS["cases whose anywhere plan severs a link"] and 4 * differing >= 3 * cases


def test_the_census_reaches_its_floors(plans):
    counts = collections.Counter()
    counts["kept cases"] = len(plans)
    for planned in plans.values():
        drawn = planned.drawn
        counts["cases with a forward same-group link over a segment boundary"] += len(planned.links) > 0
        counts["forward same-group links over a segment boundary"] += len(planned.links)
        census = {name: ss.plan_census(planned, one) for name, one in planned.plans.items()}
        counts["cases whose anywhere plan severs a link"] += census["anywhere"]["severed links"] > 0
        counts["cases whose seams plan has a cut between groups"] += census["seams"]["cuts between groups"] > 0
        world = planned.plans["seams"].world
        counts["series-order cases cut by series_range"] += world is not None
        counts["series-order cases with more ranks than series"] += world is not None and world > len(drawn.kinds)
        counts["ranks without a series"] += census["seams"]["ranks without a series"]
        tail = range(len(drawn.batch) - drawn.n_tail, len(drawn.batch))
        beside = any(cut in tail or cut - 1 in tail for cut in planned.plans["anywhere"].cuts)
        assert beside == (drawn.n_tail > 0)
        counts["cases whose anywhere plan cuts beside a single-point tail segment"] += beside
        kept = sum(ss.trend_request_kept(planned, request) for request in planned.trend_requests)
        counts["trend requests whose x stays below 2^53 (kept)"] += kept
        counts["trend requests left out"] += len(planned.trend_requests) - kept
        for request in planned.sample_requests:
            if request.style == "signed_zero":
                counts["cases with a sample request through a row that holds -0.0"] += 1
                one_row, wide = ls.own_grid_rows(drawn, request)
                single = one_row & (ls.reference_sample(drawn, request, sc.EXACT)["count"] == 1)
                counts["sample cells whose one contribution is a row that holds -0.0"] += \
                    int((wide[single].view(np.uint64) == 1 << 63).sum())
        for one in census.values():
            counts["plans with an empty shard"] += one["empty shards"] > 0
            counts["shards that begin or end with a single-point segment"] += \
                one["shards that begin or end with a single-point segment"]
            counts["shards without a row of some group"] += one["shards without a row of some group"]
    for name, count in sorted(counts.items()):
        print(f"{name}: {count}")
    short = {name: (counts[name], floor) for name, floor in FLOORS.items() if counts[name] < floor}
    assert not short, short
    assert 10 * counts["trend requests left out"] <= counts["trend requests whose x stays below 2^53 (kept)"]


MERGES = (("agg_merge_n", mdb.fresh_agg_states), ("m4_merge", mdb.fresh_m4_cells), ("moments_merge", mdb.fresh_moments_cells),
          ("comoments_merge", mdb.fresh_comoments_cells), ("integral_merge", mdb.fresh_integral_cells),
          ("sample_merge", mdb.fresh_sample_cells), ("change_merge", mdb.fresh_change_cells),
          ("dwell_merge", lambda shape: np.zeros(shape, dtype=np.uint64)))


@pytest.mark.parametrize("name,fresh", MERGES)
def test_the_host_folds_exist_and_refuse_two_sizes(name, fresh):
    merge = getattr(mdb, name)
    into = fresh((2, 3))
    assert merge(into, fresh((2, 3))) is into and into.tobytes() == fresh((2, 3)).tobytes()
    with pytest.raises(ValueError):
        merge(into, fresh((2, 2)))
    with pytest.raises(ValueError):
        merge(fresh((3,)), fresh((2, 3)))
    with pytest.raises(ValueError):
        merge(into, np.zeros((2, 3)))
    assert into.tobytes() == fresh((2, 3)).tobytes()
