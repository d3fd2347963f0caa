"""Randomised differential soak of dwell_buckets over the cases of tests/linked_soak.py - the hostile input domain of
tests/query_soak.py under three groupings, tails of single-point segments with equal timestamps, seven kinds of max_gap,
bucket requests far below the data (the saturating bucket ends), a microsecond beside a row and dense enough to cut most
links - with the edge list of the same index's tests/query_soak.py case: edges drawn from the data's own values, NaN,
infinities and both zeros among them.

Every request of a case - its own, far, near and dense - runs through the host form and twice through the dev form on
one uploaded batch; where the case has list cuts, also through the list form on those slices (links cross the cuts).
Every result is compared with the reference (tests/dwell_cases.py over the case's linked intervals) exactly: the
operator is integer arithmetic. The only cases left out are those linked_soak.draw returns None for (more than 8 192
rows; tests/test_linked_soak_cpu.py holds them to at most a third of the indices).

MDB_LINKED_SOAK_CASES sets the number of indices (default 60). Every case is a pure function of its index."""

import os

import numpy as np
import pytest

import dwell_cases as dc
import linked_soak as ls
import query_soak as qs

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("MDB_LINKED_SOAK_CASES", "60"))
BLOCK = 20  # indices per pytest item
BLOCKS = range((N_CASES + BLOCK - 1) // BLOCK)


def run_case(hip, index, census):
    """One case through every form; False when the case is left out for its size."""
    drawn = ls.draw(index)
    if drawn is None:
        return False
    edges = qs.make_case(index).edges
    dev = hip.upload_segments(drawn.batch)
    try:
        for request in drawn.requests:
            where = f"linked soak case {index} ({drawn.grouping}, tail {drawn.n_tail}), {len(edges)} edges, {ls.describe(request)}"
            args = (edges, request.origin, request.width, request.n_buckets)
            common = dict(max_gap=request.max_gap, n_groups=drawn.n_groups)
            expected = dc.cells_of(ls.linked(drawn, request.max_gap), edges, drawn.n_groups, *args[1:])
            forms = [("host", hip.dwell_buckets(drawn.batch, *args, groups=drawn.groups, **common)),
                     ("dev", hip.dwell_buckets_dev(dev, *args, groups=drawn.groups, **common)),
                     ("dev again", hip.dwell_buckets_dev(dev, *args, groups=drawn.groups, **common))]
            if drawn.list_cuts is not None:
                batches, groups = ls.slices(drawn)
                forms.append(("list", hip.dwell_buckets_list(batches, *args, groups=groups, **common)))
            for form, got in forms:
                np.testing.assert_array_equal(got, expected, err_msg=f"{where}, {form}")
            census["requests"] += 1
            census["cells"] += int((expected > 0).sum())
            census["microseconds"] += int(expected.sum(dtype=object))
    finally:
        dev.free()
        qs.forget_grids()
    census["cases"] += 1
    return True


@pytest.mark.parametrize("block", BLOCKS)
def test_dwell_buckets(hip, block):
    census = {"cases": 0, "requests": 0, "cells": 0, "microseconds": 0}
    last = min(N_CASES, (block + 1) * BLOCK)
    for index in range(block * BLOCK, last):
        run_case(hip, index, census)
    print(f"dwell, indices {block * BLOCK} to {last - 1}: {census['cases']} cases, {census['requests']} requests, "
          f"{census['cells']} cells with a non-zero duration, {census['microseconds']} microseconds in all")
    assert census["cases"] >= (last - block * BLOCK) // 2 and census["cells"] > 0

