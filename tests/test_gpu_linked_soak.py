"""Randomised differential soak of the four linked-row operators - integral_buckets, sample_at, change_buckets and
episodes - over the cases of tests/linked_soak.py: the hostile input domain of tests/query_soak.py under three
groupings, tails of single-point segments with equal timestamps, seven kinds of max_gap, bucket requests far below the
data, a microsecond beside a row and dense enough to cut most links, a series' own grid, and slices of 1 to 1 000 pairs
or points.

Every operator runs through its host form and twice through its dev form on one uploaded batch; where the case has
list cuts, also through its list form on those slices (links and episodes cross the cuts). Each result is held to the
operator's own reference under the operator's own rule (integral_cases / sample_cases / change_cases.assert_cells,
episodes_cases.assert_episodes: no tolerance is set here); integer members have the same bytes in every form. The
results are also checked against each other: change_buckets' durations against integral_buckets', the episodes'
counts against n_passing, sample_at's EXACT counts against its LINEAR ones.

MDB_LINKED_SOAK_CASES sets the number of indices (default 60; an index whose case has more than 8 192 rows is left out);
the long run is recorded in DESIGN.md section 2. Every case is a pure function of its index:
scripts/debug_linked_soak_case.py INDEX [operator] replays one."""

import contextlib
import os

import numpy as np
import pytest

import change_cases as chc
import episodes_cases as ec
import integral_cases as ic
import linked_soak as ls
import query_soak as qs
import sample_cases as sc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import _abi

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("MDB_LINKED_SOAK_CASES", "60"))
BLOCK = 20  # indices per pytest item
BLOCKS = range((N_CASES + BLOCK - 1) // BLOCK)
PAIRS_SWITCH, POINTS_SWITCH = "MDB_AGG_BUCKET_SLICE_PAIRS", "MDB_FILTER_SLICE_POINTS"


@contextlib.contextmanager
def _environment(name, value):
    """The switch in the environment (the binding has the library read it again before every call), put back after."""
    before = os.environ.get(name)
    if value is not None:
        os.environ[name] = str(value)
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = before


@contextlib.contextmanager
def _option(hip, name, value):
    """The switch set in the library itself, as tests/test_gpu_change.py sets it: no reload may put the environment's
    value back meanwhile."""
    if value is None:
        yield
        return
    reloading = _abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL
    try:
        _abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL = False
        assert hip.lib.mdb_set_option(name.encode(), str(value).encode()) == 0
        yield
    finally:
        hip.lib.mdb_set_option(name.encode(), None)
        _abi.RELOAD_OPTIONS_BEFORE_EVERY_CALL = reloading


def _forms(drawn, dev, host, on_device, listed):
    """[(form, result)]: the host form, the dev form twice, the list form where the case has slices."""
    out = [("host", host(drawn.batch, drawn.groups)), ("dev", on_device(dev, drawn.groups)),
           ("dev again", on_device(dev, drawn.groups))]
    if drawn.list_cuts is not None:
        out.append(("list", listed(*ls.slices(drawn))))
    return out


def _same_bytes(forms, members, tell):
    for form, result in forms[1:]:
        for member in members:
            if result[member].tobytes() != forms[0][1][member].tobytes():
                tell(form, [f"{member} differs from the {forms[0][0]} form's bytes"])


class _Census:
    def __init__(self):
        self.checked = self.non_finite = 0

    def add(self, checked, non_finite):
        self.checked += checked
        self.non_finite += non_finite


def _integral(hip, drawn, dev, tell, census):
    with _environment(PAIRS_SWITCH, drawn.slice_pairs):
        for request in drawn.requests:
            window = (request.origin, request.width, request.n_buckets)
            for method, name in ls.INTEGRAL_METHODS:
                common = dict(method=method, max_gap=request.max_gap, n_groups=drawn.n_groups)
                forms = _forms(drawn, dev, lambda b, g: hip.integral_buckets(b, *window, groups=g, **common),
                               lambda d, g: hip.integral_buckets_dev(d, *window, groups=g, **common),
                               lambda bs, gs: hip.integral_buckets_list(bs, *window, groups=gs, **common))
                expected = ls.reference_integral(drawn, request, method)
                for form, got in forms:
                    differences, plain, special = ls.held(ic.assert_cells, got, expected, name)
                    tell(request, f"{name}, {form}", differences)
                    if form == "host":
                        census.add(plain, special)
                _same_bytes(forms, ("duration",), lambda form, d: tell(request, f"{name}, {form}", d))


def _sample(hip, drawn, dev, tell, census):
    with _environment(PAIRS_SWITCH, drawn.slice_pairs):
        for request in drawn.sample_requests:
            window = (request.origin, request.width, request.n_buckets)
            counts = {}
            for method, name in ls.SAMPLE_METHODS:
                common = dict(method=method, max_gap=request.max_gap, n_groups=drawn.n_groups)
                forms = _forms(drawn, dev, lambda b, g: hip.sample_at(b, *window, groups=g, **common),
                               lambda d, g: hip.sample_at_dev(d, *window, groups=g, **common),
                               lambda bs, gs: hip.sample_at_list(bs, *window, groups=gs, **common))
                expected = ls.reference_sample(drawn, request, method)
                for form, got in forms:
                    differences, plain, special = ls.held(sc.assert_cells, got, expected, name)
                    if request.style == "own_grid":
                        differences += ls.own_grid_differences(drawn, request, got, expected)[0]
                    tell(request, f"{name}, {form}", differences)
                    if form == "host":
                        census.add(plain, special)
                _same_bytes(forms, ("count",), lambda form, d: tell(request, f"{name}, {form}", d))
                counts[method] = forms[0][1]["count"]
            if (counts[sc.EXACT] > counts[sc.LINEAR]).any():
                tell(request, "exact against linear", ["a cell's EXACT count exceeds its LINEAR count"])


def _change(hip, drawn, dev, tell, census):
    first, last = int(drawn.timestamps.min()), int(drawn.timestamps.max())
    with _option(hip, PAIRS_SWITCH, drawn.slice_pairs):
        for request in drawn.requests:
            window = (request.origin, request.width, request.n_buckets)
            common = dict(max_gap=request.max_gap, n_groups=drawn.n_groups)
            forms = _forms(drawn, dev, lambda b, g: hip.change_buckets(b, *window, groups=g, **common),
                           lambda d, g: hip.change_buckets_dev(d, *window, groups=g, **common),
                           lambda bs, gs: hip.change_buckets_list(bs, *window, groups=gs, **common))
            expected = ls.reference_change(drawn, request)
            for form, got in forms:
                differences, plain, poisoned = ls.held(chc.assert_cells, got, expected, form)
                tell(request, form, differences)
                if form == "host":
                    census.add(plain, poisoned)
            _same_bytes(forms, ("count", "n_fall", "duration"), lambda form, d: tell(request, form, d))
            if request.origin <= first and last < request.origin + request.n_buckets * request.width:
                # the window covers the data: both operators see every linked pair whole, so the linked time of a
                # group is one number (tests/test_gpu_change.py: test_durations_agree_with_the_time_weighted_operator)
                integral = hip.integral_buckets(drawn.batch, *window, groups=drawn.groups, method=mdb.MDB_INTEGRAL_STEP,
                                                **common)
                ours = [sum(int(x) for x in row) % (1 << 64) for row in forms[0][1]["duration"]]
                theirs = [sum(int(x) for x in row) % (1 << 64) for row in integral["duration"]]
                if ours != theirs:
                    tell(request, "durations against integral_buckets", [f"per group {ours} != {theirs}"])


def _episodes(hip, drawn, dev, tell, census):
    flt = ls.value_filter(drawn)
    with _environment(POINTS_SWITCH, drawn.slice_points):
        for rule in drawn.episodes:
            common = dict(n_groups=drawn.n_groups, max_gap=rule.max_gap, min_duration=rule.min_duration,
                          min_count=rule.min_count)
            forms = _forms(drawn, dev, lambda b, g: hip.episodes(b, flt, g, **common),
                           lambda d, g: hip.episodes_dev(d, flt, g, **common),
                           lambda bs, gs: hip.episodes_list(bs, flt, gs, **common))
            expected, magnitudes, n_rows, n_passing, _ = ls.reference_episodes(drawn, rule)
            for form, (got, got_rows, got_passing) in forms:
                differences = qs.exact_differences(np.array([got_rows, got_passing]), np.array([n_rows, n_passing]),
                                                   "(n_rows, n_passing)")
                tell(rule, form, differences + ls.episodes_differences(got, expected, magnitudes))
                if not ec.same_but_sum(got, forms[0][1][0]):
                    tell(rule, form, [f"a member other than sum differs from the {forms[0][0]} form's bytes"])
            census.add(int(np.isfinite(expected["sum"]).sum()), int((~np.isfinite(expected["sum"])).sum()))
            # without the two minimum filters every passing row lies in exactly one episode
            every, _, passing = hip.episodes(drawn.batch, flt, drawn.groups, **dict(common, min_duration=0, min_count=0))
            if int(every["count"].sum()) != passing or passing != n_passing:
                tell(rule, "counts against n_passing", [f"the counts sum to {int(every['count'].sum())}, n_passing is "
                                                        f"{passing}, the reference's {n_passing}"])


OPERATORS = {"integral": _integral, "sample": _sample, "change": _change, "episodes": _episodes}


def _describe(what):
    if hasattr(what, "style"):
        return ls.describe(what)
    return f"max_gap {what.max_gap} ({what.gap_choice}), min_count {what.min_count}, min_duration {what.min_duration}"


def run_case(hip, index, operator, census, report=None):
    """One case through every form of one operator. `report(where, operator, form, differences)` receives every
    comparison (the debug script's); without it the first difference fails the test, named by case, operator, request and
    form. Returns False when the case is left out for its size."""
    drawn = ls.draw(index)
    if drawn is None:
        return False

    def tell(what, form, differences):
        where = f"linked soak case {index} ({drawn.grouping}, tail {drawn.n_tail}), {_describe(what)}"
        if report is not None:
            report(where, operator, form, differences)
        else:
            assert not differences, (where, operator, form, differences[:5])

    dev = hip.upload_segments(drawn.batch)
    try:
        OPERATORS[operator](hip, drawn, dev, tell, census)
    finally:
        dev.free()
        qs.forget_grids()
    return True


def _run_block(hip, block, operator, what):
    census = _Census()
    for index in range(block * BLOCK, min(N_CASES, (block + 1) * BLOCK)):
        run_case(hip, index, operator, census)
    print(f"{operator}, indices {block * BLOCK} to {min(N_CASES, (block + 1) * BLOCK) - 1}: {census.checked} {what} "
          f"checked numerically, {census.non_finite} only have to be non-finite")
    assert census.checked > 10 * census.non_finite


@pytest.mark.parametrize("block", BLOCKS)
def test_integral_buckets(hip, block):
    _run_block(hip, block, "integral", "cells")


@pytest.mark.parametrize("block", BLOCKS)
def test_sample_at(hip, block):
    _run_block(hip, block, "sample", "cells")


@pytest.mark.parametrize("block", BLOCKS)
def test_change_buckets(hip, block):
    _run_block(hip, block, "change", "cells")


@pytest.mark.parametrize("block", BLOCKS)
def test_episodes(hip, block):
    _run_block(hip, block, "episodes", "episodes' sums")


def test_cases_that_once_failed(hip):
    for index, operator in ():
        run_case(hip, index, operator, _Census())
