"""The generator of the linked-row operators' soak (tests/linked_soak.py), held to its promises without a GPU over the
indices 0 to 199: draw() is a pure function of its index; only the size filter leaves a case out, and at most a third
of them; every model type, kind of timestamps, grouping, max_gap choice and request style occurs; the census of what the
cases hold reaches its floors; and the four references run on every drawn case, so an assertion of a reference's own
(change_cases.cells_of's len(signs) == 1, episodes_cases.reference's starts and ends) is met here and not on the GPU."""

import collections

import numpy as np
import pytest

import linked_soak as ls
import query_soak as qs
import sample_cases as sc
import modelardb_rs_amd as mdb

N_INDICES = 200
# What the cases of the indices 0 .. 199 must hold at least. The cells are counted over every run the GPU tier makes
# (integral: two methods, sample: three, episodes: twelve rules).
FLOORS = {
    "finite integral cells": 80_000,
    "non-finite integral cells": 100,
    "finite sample cells": 150_000,
    "non-finite sample cells": 50,
    "poisoned change cells": 25,
    "episodes that span two or more segments": 500,
    "seam links": 250,
    "backward steps inside a group": 80,
    "linked intervals that cross a bucket edge": 15_000,
    "pairs of consecutive same-group rows with equal timestamps": 20,
    "own-grid sample cells with count == 1": 10_000,
}


@pytest.fixture(scope="module")
def census():
    """(what occurred, the counts, the indices left out), from the references of every drawn case."""
    seen, counts, left_out = set(), collections.Counter(), []
    for index in range(N_INDICES):
        drawn = ls.draw(index)
        if drawn is None:
            assert len(qs.make_case(index).timestamps) > ls.MAX_ROWS   # (the only reason)
            left_out.append(index)
            continue
        assert len(drawn.timestamps) <= ls.MAX_ROWS + 5
        seen |= {("model", mdb.MODEL_TYPE_NAMES[t]) for t in set(drawn.batch.model_type_id.tolist())}
        seen |= {("timestamps", kind) for kind in drawn.kinds} | {("grouping", drawn.grouping)}
        seen |= {("request", request.style) for request in drawn.sample_requests}
        seen |= {("max_gap", request.gap_choice) for request in drawn.sample_requests}
        seen |= {("max_gap", rule.gap_choice) for rule in drawn.episodes}
        seen |= {("tail", drawn.n_tail > 0), ("list cuts", drawn.list_cuts is not None),
                 ("slices", drawn.slice_pairs), ("slices of points", drawn.slice_points), ("permuted", drawn.permuted)}
        rows = ls.row_census(drawn)
        counts["seam links"] += rows["seam links"]
        counts["backward steps inside a group"] += rows["backward steps"]
        counts["pairs of consecutive same-group rows with equal timestamps"] += rows["equal timestamps"]
        assert drawn.n_tail > 0 or drawn.grouping != "series" or rows["equal timestamps"] == 0   # (the generator makes no tie)
        for request in drawn.requests:
            assert request.width >= 1 and 1 <= drawn.n_groups * request.n_buckets <= qs.MAX_CELLS, index
            for method, _ in ls.INTEGRAL_METHODS:
                expected = ls.reference_integral(drawn, request, method)
                hit = expected["duration"] > 0
                counts["finite integral cells"] += int((hit & expected["finite"]).sum())
                counts["non-finite integral cells"] += int((hit & ~expected["finite"]).sum())
            expected = ls.reference_change(drawn, request)
            counts["plain change cells"] += int(((expected["count"] > 0) & ~expected["poisoned"]).sum())
            counts["poisoned change cells"] += int(expected["poisoned"].sum())
            counts["linked intervals that cross a bucket edge"] += ls.edge_crossings(drawn, request)
        for request in drawn.sample_requests:
            assert 1 <= drawn.n_groups * request.n_buckets <= qs.MAX_CELLS, index
            for method, _ in ls.SAMPLE_METHODS:
                expected = ls.reference_sample(drawn, request, method)
                hit = expected["count"] > 0
                counts["finite sample cells"] += int((hit & expected["finite"]).sum())
                counts["non-finite sample cells"] += int((hit & ~expected["finite"]).sum())
                if request.style == "own_grid" and method == sc.LINEAR:
                    one_row, _ = ls.own_grid_rows(drawn, request)
                    counts["own-grid sample cells with count == 1"] += int((one_row & (expected["count"] == 1)).sum())
        for rule in drawn.episodes:
            episodes, _, _, n_passing, _ = ls.reference_episodes(drawn, rule)
            counts["episodes"] += len(episodes)
            counts["episodes that span two or more segments"] += ls.episodes_over_segments(drawn, episodes)
            every = ls.reference_episodes(drawn, rule, min_count=0, min_duration=0)[0]
            assert int(every["count"].sum()) == n_passing, index
        qs.forget_grids()
    return seen, counts, left_out


def test_a_case_is_a_pure_function_of_its_index():
    drawn = [index for index in (0, 1, 7, 15, 33, 59, 1234) if ls.draw(index) is not None]
    assert len(drawn) >= 4
    for index in drawn:
        assert ls.case_bytes(ls.draw(index)) == ls.case_bytes(ls.draw(index)), index
    assert ls.case_bytes(ls.draw(drawn[0])) != ls.case_bytes(ls.draw(drawn[1]))


def test_only_the_size_filter_leaves_cases_out(census):
    _, _, left_out = census
    print(f"{len(left_out)} of {N_INDICES} indices left out for more than {ls.MAX_ROWS} rows")
    assert 3 * len(left_out) <= N_INDICES, left_out


def test_every_kind_of_case_occurs(census):
    seen, _, _ = census
    wanted = {("model", name) for name in mdb.MODEL_TYPE_NAMES} | \
        {("timestamps", kind) for kind in ("regular", "irregular", "gaps")} | \
        {("grouping", name) for name in ls.GROUPINGS} | {("max_gap", name) for name in ls.GAP_CHOICES} | \
        {("request", style) for style in ls.STYLES + ("own_grid",)} | \
        {("tail", True), ("tail", False), ("list cuts", True), ("list cuts", False), ("permuted", True),
         ("permuted", False), ("slices", None), ("slices of points", None)} | \
        {("slices", n) for n in ls.SLICE_PAIRS} | {("slices of points", n) for n in ls.SLICE_POINTS}
    assert not wanted - seen, sorted(map(str, wanted - seen))


def test_the_census_reaches_its_floors(census):
    _, counts, _ = census
    for name, count in sorted(counts.items()):
        print(f"{name}: {count}")
    short = {name: (counts[name], floor) for name, floor in FLOORS.items() if counts[name] < floor}
    assert not short, short
    # the cells that only have to be non-finite must not carry the test
    assert counts["finite integral cells"] > 10 * counts["non-finite integral cells"]
    assert counts["finite sample cells"] > 10 * counts["non-finite sample cells"]
    assert counts["plain change cells"] > 10 * counts["poisoned change cells"]


def test_the_own_grid_cells_are_the_rows(census):
    """own_grid_rows against sample_cases.sample_rows under EXACT: a cell the helper says holds one row has count 1 and
    that row's value as its exact sum."""
    checked = 0
    for index in range(40):
        drawn = ls.draw(index)
        for request in ([] if drawn is None else drawn.sample_requests):
            if request.style != "own_grid":
                continue
            one_row, wide = ls.own_grid_rows(drawn, request)
            expected = ls.reference_sample(drawn, request, sc.EXACT)
            assert ((expected["count"] == 1) == one_row).all(), index
            for where in zip(*np.nonzero(one_row & expected["finite"])):
                assert float(expected["sum"][where]) == wide[where], (index, where)
                checked += 1
    assert checked > 1000
