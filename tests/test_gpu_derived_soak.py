"""Randomised differential soak of the derived-field operator over the cases of tests/pair_soak.py::draw, imported
unchanged: the hostile input domain of tests/test_gpu_soak.py in an x field (permuted in half the cases, under three
groupings) against a y field compressed on its own, of six kinds, with tails of single-point segments, time ranges that
cut segments, buckets far below the data, a microsecond wide and dense, list cuts that differ per field and slices of 1
to 1 000 pairs.

Only the exact members are compared, on every case, every request and every cell, nothing left out: the z column bit
for bit (host form and device form) and count, min and max of every cell (min and max with ==, mdb.h), through the host
form, the dev form and - where the case has list cuts - the list form, which all give the same bytes. mean and m2 are
not judged here: on these domains their conditioning is a study of its own, as tests/pair_soak.py shows.

MDB_DERIVED_SOAK_CASES sets the number of indices (default 80; an index whose case has more than 8 192 rows is left
out). Every case is a pure function of its index."""

import os

import numpy as np
import pytest

import derived_cases as dc
import pair_soak as ps
import modelardb_rs_amd as mdb
from test_gpu_linked_soak import PAIRS_SWITCH, _option

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("MDB_DERIVED_SOAK_CASES", "80"))
BLOCK = 20
BLOCKS = range((N_CASES + BLOCK - 1) // BLOCK)
NAMES = list(dc.EXPRESSIONS)


def _same_bits(got, expected):
    return got.shape == expected.shape and bool(((got.view(np.uint32) == expected.view(np.uint32)) | (np.isnan(got) & np.isnan(expected))).all())


@pytest.mark.parametrize("block", BLOCKS)
def test_exact_members_on_hostile_cases(hip, block):
    cases_run = cells_compared = rows_compared = 0
    for index in range(block * BLOCK, min((block + 1) * BLOCK, N_CASES)):
        drawn = ps.draw(index)
        if drawn is None:
            continue
        cases_run += 1
        dev_x = hip.upload_segments(drawn.x.batch)
        dev_y = dev_x if drawn.y is drawn.x else hip.upload_segments(drawn.y.batch)
        try:
            for k, request in enumerate(drawn.requests):
                name = NAMES[(index + k) % len(NAMES)]
                expr = dc.expression(name)
                context = f"case {index} ({drawn.kind}) {name} {ps.describe(request)}"
                t_lo, t_hi = ps.time_bounds(request)
                ts, z = dc.column(drawn.x, drawn.y, name, t_lo, t_hi)
                got_ts, got = hip.derived_values(drawn.x.batch, drawn.y.batch, expr, t_lo, t_hi)
                assert np.array_equal(got_ts, ts) and _same_bits(got, z), context
                dev_values = hip.dev_alloc(4 * (len(z) + 2))
                try:   # (one float off a 16-byte boundary, no timestamps)
                    assert hip.derived_values_dev(dev_x, dev_y, expr, t_lo, t_hi, None, dev_values + 4, len(z)) == len(z)
                    assert _same_bits(hip.download_array(dev_values, len(z) + 1, np.float32)[1:], z), context
                finally:
                    hip.dev_free(dev_values)
                rows_compared += 2 * len(z)
                args, ranged = ps.window(request)
                common = dict(ranged, n_groups=drawn.n_groups)
                expected = dc.oracle(drawn.x, drawn.y, name, drawn.groups, drawn.n_groups, *args, t_lo, t_hi)
                with _option(hip, PAIRS_SWITCH, drawn.slice_pairs):
                    forms = [hip.derived_buckets(drawn.x.batch, drawn.y.batch, expr, *args, groups=drawn.groups, **common),
                             hip.derived_buckets_dev(dev_x, dev_y, expr, *args, groups=drawn.groups, **common)]
                    if drawn.x_cuts is not None:
                        xs, ys, groups = ps.slices(drawn)
                        forms.append(hip.derived_buckets_list(xs, ys, expr, *args, groups=groups, **common))
                dc.assert_exact_members(forms[0], expected, context)
                for other in forms[1:]:
                    assert other.tobytes() == forms[0].tobytes(), context
                counts = hip.agg_buckets(drawn.x.batch, *args, groups=drawn.groups, **common)
                np.testing.assert_array_equal(forms[0]["count"], counts["count"], err_msg=context)
                cells_compared += forms[0].size
        finally:
            dev_x.free()
            if dev_y is not dev_x:
                dev_y.free()
    print(f"block {block}: {cases_run} cases, {rows_compared} rows of z and {cells_compared} cells compared exactly")
    assert cases_run > 0
