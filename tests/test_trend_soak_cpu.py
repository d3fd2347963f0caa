"""The cases of the trend operator's soak (tests/test_gpu_trend_soak.py), held to account without a GPU: draw() is a pure
function of its index, and the 200 drawn cases hold what the soak exists for - all three model types, regular and
irregular timestamps, a bucket width above 2^40, an origin below -2^62, cells of one point - with most of the cells
open to the numeric check. The generator is then known to reach them before anyone trusts the GPU run."""

import numpy as np
import pytest

import modelardb_rs_amd as mdb
import query_soak as qs
import test_gpu_trend_soak as trend_soak


@pytest.fixture(scope="module")
def drawn():
    """[(case, requests, references)] of the 200 cases, computed once."""
    out = []
    for index in range(trend_soak.N_CASES):
        case, requests = trend_soak.draw(index)
        out.append((case, requests, [trend_soak.reference(case, request) for request in requests]))
        qs.forget_grids()
    return out


def test_a_draw_is_a_pure_function_of_its_index():
    for index in (0, 7, 199):
        one, other = trend_soak.draw(index), trend_soak.draw(index)
        assert qs.case_bytes(one[0]) == qs.case_bytes(other[0])
        assert [vars(request) for request in one[1]] == [vars(request) for request in other[1]]
        assert len(one[1]) == len(one[0].requests) + 2


def test_census_of_the_drawn_cases(drawn):
    assert len(drawn) == 200
    types, kinds, styles = set(), set(), set()
    widest, lowest, one_point, wide_cells, checked, exempt = 0, 0, 0, 0, 0, 0
    for case, requests, references in drawn:
        types |= set(case.batch.model_type_id.tolist())
        kinds |= set(case.kinds)
        for request, expected in zip(requests, references):
            assert request.width >= 1 and 1 <= case.n_groups * request.n_buckets <= qs.MAX_CELLS
            assert qs.I64_MIN <= request.origin <= qs.I64_MAX
            styles.add(request.style)
            widest, lowest = max(widest, request.width), min(lowest, request.origin)
            hit = expected["count"] > 0
            one_point += int((expected["count"] == 1).sum())
            wide_cells += int(hit.sum()) if request.width > 1 << 53 else 0
            checked += int((hit & expected["finite_y"]).sum())
            exempt += int((hit & ~expected["finite_y"]).sum())
    assert types == {mdb.MDB_PMC_MEAN_ID, mdb.MDB_SWING_ID, mdb.MDB_MACAQUE_V_ID}
    assert {"regular", "irregular"} <= kinds
    assert styles == set(qs.STYLES) | {"far", "near"}
    assert widest > 1 << 40 and lowest < -(1 << 62)
    assert one_point > 100 and wide_cells > 100
    print(f"{checked} cells open to the numeric check, {exempt} hold a NaN or an infinity, {one_point} of one point, "
          f"{wide_cells} in buckets wider than 2^53")
    assert checked > 10 * exempt and checked > 10_000
