"""A randomised differential soak of the trend operator (mdb_trend_buckets*): 200 cases drawn from tests/query_soak.py's
generators - value levels from 1e-38 to 3e37 with NaN, infinities, zeros and subnormals, epoch-scale and negative
timestamps, intervals of 1 and 60 000 000, gaps up to 2^41, random error bounds, chunk cuts and row orders - under the
case's own bucket requests and two more that put the ORIGIN where the x arithmetic can go wrong: far below the data
(down to the low end of int64, widths of 2^41, 2^54 and 2^62 and beyond) and a microsecond either side of a timestamp.

The reference is point by point: x = (t - origin) - bucket * width in integers, dx = x - x_first (an integer below
2^53), and each cell in exact arithmetic (comoments_cases.cell_reference on (dx, v), math.fsum). No case is skipped.
Assertions are comoments_cases.assert_cells: the only cells exempt from the numeric check are those that hold a NaN or an
infinity, whose mean_y, m2_y and c_xy must be non-finite; a cell of a bucket wider than 2^53 is held to the same
tolerances, its mean_x within 2^-44 of its largest |x| (a relative bound: x itself rounds there when it is converted).

tests/test_trend_soak_cpu.py asserts without a GPU that these cases hold what the soak exists for."""

import pytest

import comoments_cases as cc
import query_soak as qs

pytestmark = pytest.mark.gpu

from trend_soak import FAR_WIDTHS, I64_MAX, I64_MIN, N_CASES, SEED, draw, reference   # noqa: F401 (moved there, unchanged)


def _run(hip, case, request, monkeypatch):
    args = (request.origin, request.width, request.n_buckets)
    kwargs = dict(t_lo=request.t_lo, t_hi=request.t_hi, n_groups=case.n_groups)
    if case.slice_pairs:
        monkeypatch.setenv("MDB_AGG_BUCKET_SLICE_PAIRS", "1000")
    try:
        if case.list_cuts is None:
            return hip.trend_buckets(case.batch, *args, groups=case.groups, **kwargs)
        cuts = [0] + case.list_cuts + [len(case.batch)]
        return hip.trend_buckets_list([case.batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])], *args,
                                      groups=[case.groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])], **kwargs)
    finally:
        if case.slice_pairs:
            monkeypatch.delenv("MDB_AGG_BUCKET_SLICE_PAIRS")


def test_two_hundred_cases_against_the_points(hip, monkeypatch):
    checked = exempt = 0
    for index in range(N_CASES):
        case, requests = draw(index)
        for request in requests:
            got = _run(hip, case, request, monkeypatch)
            expected = reference(case, request)
            cc.assert_cells(got, expected, f"case {index} {request.style} {request.origin} {request.width}")
            hit = expected["count"] > 0
            checked += int((hit & expected["finite_y"]).sum())
            exempt += int((hit & ~expected["finite_y"]).sum())
        qs.forget_grids()
    print(f"{checked} cells checked numerically, {exempt} hold a NaN or an infinity")
    assert checked > 10 * exempt and checked > 10_000

