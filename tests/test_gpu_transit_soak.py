"""Randomised differential soak of transit_buckets over the cases of tests/linked_soak.py - the hostile input domain of
tests/query_soak.py under three groupings, tails of single-point segments with equal timestamps, seven kinds of max_gap,
bucket requests far below the data (the saturating bucket ends), a microsecond beside a row and dense enough to cut most
links - with the edge list of the same index's tests/query_soak.py case: edges drawn from the data's own values, NaN,
infinities and both zeros among them.

Every request of a case - its own, far, near and dense - runs through the host form and twice through the dev form on
one uploaded batch; where the case has list cuts, also through the list form on those slices (pairs cross the cuts).
Every result is compared with the reference (tests/transit_cases.py over the case's linked intervals) exactly: the
operator counts. The only cases left out are those linked_soak.draw returns None for (more than 8 192 rows;
tests/test_linked_soak_cpu.py holds them to at most a third of the indices).

With the reference rule alone, indices 0 to 59 give 44 cases (16 left out for their size), 240 requests, 90 008 pairs
inside the buckets, 20 473 of them off the diagonal, 16 806 non-zero counters, at most 55 edges and a largest array of
6 416 256 counters (51 MB).

MDB_LINKED_SOAK_CASES sets the number of indices (default 60). Every case is a pure function of its index."""

import os

import numpy as np
import pytest

import linked_soak as ls
import query_soak as qs
import transit_cases as tc

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
            expected = tc.cells_of(ls.linked(drawn, request.max_gap), edges, drawn.n_groups, *args[1:])
            forms = [("host", hip.transit_buckets(drawn.batch, *args, groups=drawn.groups, **common)),
                     ("dev", hip.transit_buckets_dev(dev, *args, groups=drawn.groups, **common)),
                     ("dev again", hip.transit_buckets_dev(dev, *args, groups=drawn.groups, **common))]
            if drawn.list_cuts is not None:
                batches, groups = ls.slices(drawn)
                forms.append(("list", hip.transit_buckets_list(batches, *args, groups=groups, **common)))
            for form, got in forms:
                np.testing.assert_array_equal(got, expected, err_msg=f"{where}, {form}")
            pairs = int(expected.sum(dtype=object))
            census["requests"] += 1
            census["counters"] += int((expected > 0).sum())
            census["pairs"] += pairs
            census["off"] += pairs - int(np.trace(expected, axis1=2, axis2=3).sum(dtype=object))
            census["largest"] = max(census["largest"], expected.size)
            census["edges"] = max(census["edges"], len(edges))
    finally:
        dev.free()
        qs.forget_grids()
    census["cases"] += 1
    return True


@pytest.mark.parametrize("block", BLOCKS)
def test_transit_buckets(hip, block):
    census = {"cases": 0, "requests": 0, "counters": 0, "pairs": 0, "off": 0, "largest": 0, "edges": 0}
    last = min(N_CASES, (block + 1) * BLOCK)
    for index in range(block * BLOCK, last):
        run_case(hip, index, census)
    print(f"transit, indices {block * BLOCK} to {last - 1}: {census['cases']} cases, {census['requests']} requests, "
          f"{census['pairs']} pairs inside the buckets, {census['off']} of them off the diagonal, {census['counters']} "
          f"non-zero counters, at most {census['edges']} edges, the largest array {census['largest']} counters")
    assert census["cases"] >= (last - block * BLOCK) // 2 and census["pairs"] > 0 and census["off"] > 0
