"""Randomised differential soak of the query operators: the cases of tests/query_soak.py (the input domain of
tests/test_gpu_soak.py) through agg_buckets, agg_buckets_filter, agg_batch_filter, grid_batch_filter, the row masks,
hist_batch / quantile_batch, hist_buckets / quantile_buckets, m4_buckets and moments_buckets, each against the
point-by-point reference of query_soak.reference() under the rules written there.

Every operator runs through its host form and twice through its dev form on the uploaded batch (the second call reads
the cursor index the first one left: MacaqueV goes piece by piece); integer-valued outputs have the same bytes in all
three, float outputs are each held to the reference. One case in four also runs the list forms on 2 to 5 slices, one in
four runs with MDB_AGG_BUCKET_SLICE_PAIRS=1000.

MDB_QUERY_SOAK_CASES sets the number of cases (default 60); the long run is recorded in DESIGN.md section 2. Every case
is a pure function of its index: scripts/debug_query_soak_case.py INDEX replays one."""

import contextlib
import os

import numpy as np
import pytest

import modelardb_rs_amd as mdb
import query_soak as qs

pytestmark = pytest.mark.gpu

ALL = mdb.MDB_AGG_COUNT | mdb.MDB_AGG_MIN | mdb.MDB_AGG_MAX | mdb.MDB_AGG_SUM
N_CASES = int(os.environ.get("MDB_QUERY_SOAK_CASES", "60"))
BLOCK = 20  # cases per pytest item


@contextlib.contextmanager
def _environment(name, value):
    before = os.environ.get(name)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = before


def _slices(case):
    """The batch and its groups cut at the case's rows, for the list forms."""
    cuts = [0] + case.list_cuts + [len(case.batch)]
    return ([case.batch.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])],
            [case.groups[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def _forms(case, dev, host, on_device, listed=None):
    """[(form, result)]: the host form, the dev form twice, the list form where the case has slices."""
    out = [("host", host(case.batch, case.groups)), ("dev", on_device(dev, case.groups)),
           ("dev again", on_device(dev, case.groups))]
    if listed is not None and case.list_cuts is not None:
        out.append(("list", listed(*_slices(case))))
    return out


def _same_bytes(forms, pick, what, report):
    first = pick(forms[0][1])
    for form, result in forms[1:]:
        if pick(result) != first:
            report(what, form, [f"integer-valued output differs from the {forms[0][0]} form's bytes"])


def _run_request(hip, case, dev, request, expected, flt, all_pass, report):
    window = (request.origin, request.width, request.n_buckets)
    common = dict(t_lo=request.t_lo, t_hi=request.t_hi, n_groups=case.n_groups)

    agg = _forms(case, dev, lambda b, g: hip.agg_buckets(b, *window, groups=g, **common),
                 lambda d, g: hip.agg_buckets_dev(d, *window, groups=g, **common),
                 lambda bs, gs: hip.agg_buckets_list(bs, *window, groups=gs, **common))
    for form, got in agg:
        report("agg_buckets", form, qs.aggregate_differences(got, expected.agg))
    _same_bytes(agg, lambda r: r["count"].tobytes(), "agg_buckets", report)

    filtered = _forms(case, dev, lambda b, g: hip.agg_buckets_filter(b, flt, *window, groups=g, **common),
                      lambda d, g: hip.agg_buckets_filter_dev(d, flt, *window, groups=g, **common),
                      lambda bs, gs: hip.agg_buckets_filter_list(bs, flt, *window, groups=gs, **common))
    for form, got in filtered:
        report("agg_buckets_filter", form, qs.aggregate_differences(got, expected.agg_filter))
    _same_bytes(filtered, lambda r: r["count"].tobytes(), "agg_buckets_filter", report)
    passed = hip.agg_buckets_filter(case.batch, all_pass, *window, groups=case.groups, **common)
    if passed.tobytes() != agg[0][1].tobytes():
        report("agg_buckets_filter", "host", ["the all-pass filter does not give the bytes of agg_buckets"]
               + qs.aggregate_differences(passed, expected.agg, exact_zero_sign=True))

    m4_cells = _forms(case, dev, lambda b, g: hip.m4_buckets(b, *window, groups=g, **common),
                      lambda d, g: hip.m4_buckets_dev(d, *window, groups=g, **common),
                      lambda bs, gs: hip.m4_buckets_list(bs, *window, groups=gs, **common))
    for form, got in m4_cells:
        report("m4_buckets", form, qs.m4_differences(got, expected.m4))
    _same_bytes(m4_cells, lambda r: r.tobytes(), "m4_buckets", report)

    cells = _forms(case, dev, lambda b, g: hip.moments_buckets(b, *window, groups=g, **common),
                   lambda d, g: hip.moments_buckets_dev(d, *window, groups=g, **common),
                   lambda bs, gs: hip.moments_buckets_list(bs, *window, groups=gs, **common))
    for form, got in cells:
        report("moments_buckets", form, qs.moments_differences(got, expected.moments, f"case {case.index} {form}"))
    _same_bytes(cells, lambda r: r["count"].tobytes(), "moments_buckets", report)

    args = (case.edges,) + window
    counts = _forms(case, dev, lambda b, g: hip.hist_buckets(b, *args, g, request.t_lo, request.t_hi, n_groups=case.n_groups),
                    lambda d, g: hip.hist_buckets_dev(d, *args, g, request.t_lo, request.t_hi, n_groups=case.n_groups),
                    lambda bs, gs: hip.hist_buckets_list(bs, *args, gs, request.t_lo, request.t_hi, n_groups=case.n_groups))
    for form, got in counts:
        report("hist_buckets", form, qs.exact_differences(got, expected.hist, "count"))
    _same_bytes(counts, lambda r: r.tobytes(), "hist_buckets", report)

    quantiles = _forms(case, dev,
                       lambda b, g: hip.quantile_buckets(b, case.q, *window, g, request.t_lo, request.t_hi, case.n_groups),
                       lambda d, g: hip.quantile_buckets_dev(d, case.q, *window, g, request.t_lo, request.t_hi, case.n_groups))
    for form, (lo, hi, n_points) in quantiles:
        report("quantile_buckets", form, qs.quantile_differences(lo, hi, n_points, expected.quantile))
    _same_bytes(quantiles, lambda r: b"".join(part.tobytes() for part in r), "quantile_buckets", report)
    if case.interpolate:
        filled = expected.quantile.filled
        for form, (values, n_points) in (
                ("host", hip.quantile_buckets(case.batch, case.q, *window, case.groups, request.t_lo, request.t_hi,
                                              case.n_groups, interpolate=True)),
                ("dev", hip.quantile_buckets_dev(dev, case.q, *window, case.groups, request.t_lo, request.t_hi,
                                                 case.n_groups, interpolate=True))):
            report("quantile_buckets interpolated", form,
                   qs.exact_differences(n_points, expected.quantile.n_points, "n_points")
                   + qs.exact_differences(values[filled], expected.quantile.interpolated[filled], "value"))

    report("identities", "host", qs.identity_differences(agg[0][1], m4_cells[0][1], cells[0][1], counts[0][1],
                                                         quantiles[0][1], expected, case.q))


def _grid_differences(got, expected):
    out = qs.exact_differences(got[0], expected[0], "timestamp")
    out += qs.exact_differences(got[1], expected[1], "value")
    return out + qs.exact_differences(got[2], expected[2], "rows of segment")


def _run_whole_batch(hip, case, dev, expected, flt, report):
    # the filtered rows and their aggregate
    for form, got in _forms(case, dev, lambda b, g: hip.grid_filter(b, flt), lambda d, g: hip.grid_filter_resident(d, flt)):
        report("grid_batch_filter", form, _grid_differences(got, expected.filter_rows))
    states = _forms(case, dev, lambda b, g: hip.agg_filter(b, flt, ALL), lambda d, g: hip.agg_filter_dev(d, flt, ALL),
                    lambda bs, gs: hip.agg_filter_list(bs, flt, ALL))
    for form, state in states:
        report("agg_batch_filter", form, qs.aggregate_differences(qs.state_array(state), expected.filter_agg))
    _same_bytes(states, lambda s: s.count, "agg_batch_filter", report)

    # the filter as a row mask, consumed by the masked grid and the masked aggregate
    n_rows, words = len(expected.mask_bits), mdb.mask_words(len(expected.mask_bits))
    mask = hip.upload_array(np.full((words + 1) * 8, 0xFF, dtype=np.uint8))
    try:
        for form in ("dev", "dev again"):
            got_rows, got_set = hip.mask_filter_dev(dev, flt, mask, words)
            bits = hip.download_mask(mask, n_rows)
            report("mask_filter_dev", form,
                   qs.exact_differences(np.array([got_rows, got_set]), np.array([n_rows, int(expected.mask_bits.sum())]),
                                        "(n_rows, n_set)") + qs.exact_differences(bits, expected.mask_bits, "bit"))
            if (got_rows, got_set) != (n_rows, int(expected.mask_bits.sum())):
                continue   # (the consumers take n_rows and n_set on trust)
            got = hip.grid_mask_resident(dev, flt.t_lo, flt.t_hi, mask, n_rows, got_set)
            report("grid_batch_mask_dev", form, _grid_differences(got, expected.filter_rows))
            state = hip.agg_mask_dev(dev, flt.t_lo, flt.t_hi, mask, n_rows, ALL)
            report("agg_batch_mask_dev", form, qs.aggregate_differences(qs.state_array(state), expected.filter_agg))
    finally:
        hip.dev_free(mask)

    # the histogram and the quantiles under the case's time range
    t_lo, t_hi = case.time_range
    counts = _forms(case, dev, lambda b, g: hip.hist(b, case.edges, g, t_lo, t_hi, n_groups=case.n_groups),
                    lambda d, g: hip.hist_dev(d, case.edges, g, t_lo, t_hi, n_groups=case.n_groups),
                    lambda bs, gs: hip.hist_list(bs, case.edges, gs, t_lo, t_hi, n_groups=case.n_groups))
    for form, got in counts:
        report("hist_batch", form, qs.exact_differences(got, expected.hist, "count"))
    want = expected.quantile
    for form, (lo, hi, n_points) in _forms(case, dev, lambda b, g: hip.quantile(b, case.q, t_lo, t_hi),
                                           lambda d, g: hip.quantile_dev(d, case.q, t_lo, t_hi)):
        differences = qs.exact_differences(np.array(n_points), np.array(want.n_points), "n_points")
        if want.n_points:
            differences += qs.exact_differences(lo.view(np.uint32), want.lo, "lo") + \
                qs.exact_differences(hi.view(np.uint32), want.hi, "hi")
        report("quantile_batch", form, differences)
    if case.interpolate and want.n_points:
        values, _ = hip.quantile(case.batch, case.q, t_lo, t_hi, interpolate=True)
        report("quantile_batch interpolated", "host", qs.exact_differences(values, want.interpolated, "value"))


def run_case(hip, index, report=None):
    """One case through every operator. `report(operator, form, differences)` receives every comparison (the debug
    script's); without it the first difference fails the test, named by case, request, operator and form."""
    case = qs.make_case(index)
    expected = qs.reference(case)
    flt, all_pass = qs.value_filter(case), mdb.value_filter()
    where = [f"query soak case {index}"]

    def fail(operator, form, differences):
        assert not differences, (where[0], operator, form, differences[:5])

    tell = (lambda operator, form, differences: report(where[0], operator, form, differences)) if report else fail
    dev = hip.upload_segments(case.batch)
    try:
        with _environment("MDB_AGG_BUCKET_SLICE_PAIRS", "1000" if case.slice_pairs else None):
            for r, request in enumerate(case.requests):
                where[0] = f"query soak case {index}, request {r} ({request.style}: origin {request.origin}, width " \
                           f"{request.width}, {request.n_buckets} buckets, [{request.t_lo}, {request.t_hi}])"
                _run_request(hip, case, dev, request, expected.requests[r], flt, all_pass, tell)
            where[0] = f"query soak case {index}, whole batch"
            _run_whole_batch(hip, case, dev, expected, flt, tell)
    finally:
        dev.free()
        qs.forget_grids()


@pytest.mark.parametrize("block", range((N_CASES + BLOCK - 1) // BLOCK))
def test_random_cases_through_every_query_operator(hip, block):
    for index in range(block * BLOCK, min(N_CASES, (block + 1) * BLOCK)):
        run_case(hip, index)


def test_cases_that_once_failed(hip):
    for index in ():
        run_case(hip, index)
