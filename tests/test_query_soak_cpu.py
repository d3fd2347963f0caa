"""The generator and the reference of the query operators' soak (tests/query_soak.py), held to account without a GPU:
make_case() is a pure function of its index; the default 60 cases hold every shape the soak exists for (the census);
the cells that can fail are the majority; and the point-by-point reference agrees with the CPU implementations the
project already has - ora.agg_batch_range cell by cell, mdb_moments_merge_n and mdb_m4_merge_n over per-segment cells,
mdb_quantile_positions and mdb_hist_cell_of."""

import numpy as np
import pytest

import modelardb_rs_amd as mdb
import query_soak as qs
import test_gpu_agg_buckets as agg_buckets
import test_gpu_m4 as m4
import test_gpu_moments as moments

N_CASES = 60   # the default of tests/test_gpu_query_soak.py
EPOCH_US = 1_000_000_000_000_000


@pytest.fixture(scope="module")
def soak():
    """[(case, reference)] of the default cases, computed once."""
    out = []
    for index in range(N_CASES):
        case = qs.make_case(index)
        out.append((case, qs.reference(case)))
        qs.forget_grids()
    return out


def test_the_gpu_tier_runs_these_cases_by_default():
    import test_gpu_query_soak
    import os
    assert test_gpu_query_soak.N_CASES == N_CASES or "MDB_QUERY_SOAK_CASES" in os.environ


def test_a_case_is_a_pure_function_of_its_index():
    for index in (0, 1, 7, 33, 59, 1234):
        assert qs.case_bytes(qs.make_case(index)) == qs.case_bytes(qs.make_case(index)), index
    assert qs.case_bytes(qs.make_case(7)) != qs.case_bytes(qs.make_case(8))


def test_requests_stay_within_the_cap_of_cells(soak):
    for case, _ in soak:
        assert 1 <= case.n_groups <= 4 and 2 <= len(case.requests) <= 3
        for request in case.requests:
            assert request.width >= 1 and 1 <= case.n_groups * request.n_buckets <= qs.MAX_CELLS, case.index
        assert 1 <= len(case.edges) <= 64 and (np.diff(qs.hist._keys(case.edges)) > 0).all(), case.index


def _swing_segment_cut_by_a_bucket_edge(case, request):
    """A Swing segment without a residual tail whose points fall into more than one bucket of the request."""
    inside, cells = qs.place(case, request)
    swing = (case.batch.model_type_id == mdb.MDB_SWING_ID) & (case.batch.residuals.lengths() == 0)
    segment = case.segment[inside]
    of_swing = swing[segment]
    if not of_swing.any():
        return False
    segment, cells = segment[of_swing], cells[of_swing]
    low, high = np.full(len(case.batch), qs.I64_MAX), np.full(len(case.batch), -1)
    np.minimum.at(low, segment, cells)
    np.maximum.at(high, segment, cells)
    return bool((high > low).any())


def test_census_of_the_default_cases(soak):
    seen = set()
    for case, expected in soak:
        types = set(case.batch.model_type_id.tolist())
        seen |= {("model", mdb.MODEL_TYPE_NAMES[t]) for t in types}
        seen |= {("timestamps", kind) for kind in case.kinds}
        seen |= {("request", request.style) for request in case.requests}
        checks = {
            "residual tails": (case.batch.residuals.lengths() > 0).any(),
            "a negative timestamp": case.timestamps.min() < 0,
            "an epoch-scale timestamp": case.timestamps.max() >= EPOCH_US,
            "a gap of at least 2^33": case.largest_gap >= 1 << 33,
            "permuted rows": case.permuted,
            "rows in order": not case.permuted,
            "a filter that passes nothing": not expected.value_passes.any(),
            "a filter that passes everything": expected.value_passes.all(),
            "a filter that passes part": expected.value_passes.any() and not expected.value_passes.all(),
            "list forms": case.list_cuts is not None,
            "slices of 1000 pairs": case.slice_pairs,
            "interpolated quantiles": case.interpolate,
        }
        for request, wanted in zip(case.requests, expected.requests):
            hit = wanted.agg.states["count"] > 0
            checks["a cell holding NaN"] = checks.get("a cell holding NaN", False) or wanted.agg.flags["nan"].any()
            checks["a cell holding an infinity"] = checks.get("a cell holding an infinity", False) or wanted.agg.flags["inf"].any()
            checks["a cell holding both zeros"] = checks.get("a cell holding both zeros", False) or wanted.agg.flags["zeros"].any()
            checks["a bucket with exactly one point"] = checks.get("a bucket with exactly one point", False) or \
                (wanted.agg.states["count"] == 1).any()
            checks["points outside every bucket"] = checks.get("points outside every bucket", False) or \
                int(wanted.agg.states["count"].sum()) < len(case.timestamps)
            checks["a Swing segment cut by a bucket edge"] = checks.get("a Swing segment cut by a bucket edge", False) or \
                _swing_segment_cut_by_a_bucket_edge(case, request)
            assert hit.any() or request.style != "cover", case.index   # (a cover request holds every point)
        seen |= {name for name, met in checks.items() if met}
    wanted = {("model", name) for name in mdb.MODEL_TYPE_NAMES} | \
        {("timestamps", kind) for kind in ("regular", "irregular", "gaps")} | {("request", style) for style in qs.STYLES} | \
        {"residual tails", "a negative timestamp", "an epoch-scale timestamp", "a gap of at least 2^33", "permuted rows",
         "rows in order", "a filter that passes nothing", "a filter that passes everything", "a filter that passes part",
         "list forms", "slices of 1000 pairs", "interpolated quantiles", "a cell holding NaN", "a cell holding an infinity",
         "a cell holding both zeros", "a bucket with exactly one point", "points outside every bucket",
         "a Swing segment cut by a bucket edge"}
    assert not wanted - seen, sorted(map(str, wanted - seen))


def test_most_moments_cells_can_fail(soak):
    """A cell holding a NaN or an infinity only has to be non-finite: such cells must not carry the test."""
    holding = finite = 0
    for _, expected in soak:
        for wanted in expected.requests:
            hit = wanted.moments["count"] > 0
            holding += int(hit.sum())
            finite += int((hit & wanted.moments["finite"]).sum())
    print(f"{finite} of {holding} moments cells with points are finite")
    assert holding > 1000 and 2 * finite >= holding, (finite, holding)


def test_the_aggregates_agree_with_the_range_oracle_cell_by_cell(soak):
    """Requests of at most 40 cells: ora.agg_batch_range over each cell's bounds (_oracle_by_ranges) meets the SUM rule
    of the soak against the fsum of the cell's points - the rule is one the oracle satisfies with no absolute floor."""
    checked = 0
    for case, expected in soak:
        for request, wanted in zip(case.requests, expected.requests):
            if case.n_groups * request.n_buckets > 40:
                continue
            t_lo, t_hi = qs._time_bounds(request.t_lo, request.t_hi)
            ranges = agg_buckets._oracle_by_ranges(case.batch, case.groups, case.n_groups, request.origin, request.width,
                                                   request.n_buckets, t_lo, t_hi)
            differences = qs.aggregate_differences(ranges, wanted.agg)
            assert not differences, (case.index, vars(request), differences[:5])
            checked += int((wanted.agg.states["count"] > 0).sum())
    assert checked > 100, checked


def _runs(case, request):
    """The points of a request as runs of one (cell, segment) pair each, in the order of the batch's rows: (kept points,
    run number per point, cell per run)."""
    inside, cells = qs.place(case, request)
    segment = case.segment[inside]
    order = np.lexsort((np.arange(len(cells)), segment, cells))   # by cell, then segment, then position
    kept = np.flatnonzero(inside)[order]
    cells, segment = cells[order], segment[order]
    fresh = np.concatenate([[True], (cells[1:] != cells[:-1]) | (segment[1:] != segment[:-1])]) if len(cells) else np.zeros(0, bool)
    return kept, np.cumsum(fresh) - 1, cells[fresh]


def _merge_by_rounds(merge, run_cells, cell_of_run, out):
    """out[cell] = the runs of the cell merged one after the other (round k merges every cell's k-th run)."""
    if len(cell_of_run) == 0:
        return out
    first = np.concatenate([[True], cell_of_run[1:] != cell_of_run[:-1]])
    starts = np.flatnonzero(first)
    position = np.arange(len(cell_of_run)) - np.repeat(starts, np.diff(np.concatenate([starts, [len(cell_of_run)]])))
    for k in range(int(position.max()) + 1):
        rows = np.flatnonzero(position == k)
        into = np.ascontiguousarray(out[cell_of_run[rows]])
        merge(into, np.ascontiguousarray(run_cells[rows]))
        out[cell_of_run[rows]] = into
    return out


def test_m4_cells_are_the_merge_of_per_segment_reductions(soak):
    for case, expected in soak:
        for request, wanted in zip(case.requests, expected.requests):
            kept, run, cell_of_run = _runs(case, request)
            per_run = m4._reduce(case.timestamps[kept], case.values[kept], run, len(cell_of_run))
            merged = _merge_by_rounds(mdb.m4_merge, per_run, cell_of_run,
                                      mdb.fresh_m4_cells(case.n_groups * request.n_buckets))
            assert merged.tobytes() == wanted.m4.tobytes(), (case.index, vars(request))


def _moments_of_runs(values, run, n_runs):
    """The cell of every run by the run rule of mdb_moments.hpp: d = v - K with K the run's first value, s1 = sum(d),
    s2 = sum(d * d), mean = K + s1 / n, m2 = max(s2 - s1 * s1 / n, 0)."""
    cells = mdb.fresh_moments_cells(n_runs)
    if n_runs == 0:
        return cells
    starts = np.flatnonzero(np.concatenate([[True], run[1:] != run[:-1]]))
    wide = values.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = wide - wide[starts][run]
        n = np.diff(np.concatenate([starts, [len(run)]])).astype(np.float64)
        s1, s2 = np.add.reduceat(d, starts), np.add.reduceat(d * d, starts)
        m2 = s2 - s1 * s1 / n
        cells["count"], cells["mean"], cells["m2"] = n, wide[starts] + s1 / n, np.where(m2 < 0.0, 0.0, m2)
    return cells


def test_moments_cells_are_the_merge_of_per_segment_runs(soak):
    """The host arithmetic - the run rule per (segment, bucket) pair, mdb_moments_merge_n across the segments of a cell
    - meets the tolerances the kernels are held to, on every generated case."""
    for case, expected in soak:
        for request, wanted in zip(case.requests, expected.requests):
            kept, run, cell_of_run = _runs(case, request)
            per_run = _moments_of_runs(case.values[kept], run, len(cell_of_run))
            with np.errstate(invalid="ignore", over="ignore"):
                merged = _merge_by_rounds(mdb.moments_merge, per_run, cell_of_run,
                                          mdb.fresh_moments_cells(case.n_groups * request.n_buckets))
            differences = qs.moments_differences(merged.reshape(case.n_groups, request.n_buckets), wanted.moments,
                                                 f"case {case.index}")
            assert not differences, (case.index, vars(request), differences)


def test_quantile_ranks_are_those_of_mdb_quantile_positions(soak):
    pairs = set()
    for case, expected in soak:
        sizes = {int(n) for wanted in expected.requests for n in np.unique(wanted.quantile.n_points)} | \
            {expected.quantile.n_points}
        pairs |= {(x, n) for x in case.q for n in sizes if n > 0}
    assert len(pairs) > 100
    for x, n in sorted(pairs):
        rank_lo, rank_hi, fraction = mdb.quantile_positions(x, n)
        p = np.float64(x) * np.float64(n - 1)
        assert (rank_lo, rank_hi, fraction) == (int(np.floor(p)), int(np.ceil(p)), float(p - np.floor(p))), (x, n)
    # and the reference's ends are the keys at those ranks, its interpolation the rule's
    for case, expected in soak:
        wanted = expected.quantile
        for k, x in enumerate(case.q):
            if wanted.n_points == 0:
                continue
            rank_lo, rank_hi, fraction = mdb.quantile_positions(x, wanted.n_points)
            ends = qs.hist._floats_of_keys(wanted.ordered[[rank_lo, rank_hi]])
            assert (wanted.lo[k], wanted.hi[k]) == tuple(ends.view(np.uint32)), (case.index, x)
            lo, hi = float(ends[0]), float(ends[1])
            with np.errstate(invalid="ignore"):
                value = lo if wanted.lo[k] == wanted.hi[k] else lo + (hi - lo) * fraction
            assert np.array_equal(np.float64(value).view(np.uint64), wanted.interpolated[k].view(np.uint64)), (case.index, x)


def test_histogram_cells_are_those_of_mdb_hist_cell_of(soak):
    rng = np.random.default_rng(60)
    checked = 0
    for case, expected in soak:
        special = np.flatnonzero(~np.isfinite(case.values) | (case.values == 0))[:8]
        rows = np.unique(np.concatenate([rng.integers(0, len(case.values), 24), special]))
        cells = np.searchsorted(qs.hist._keys(case.edges), qs.hist._keys(case.values[rows]), side="right")
        for value, cell in zip(case.values[rows], cells):
            assert mdb.hist_cell_of(case.edges, value) == cell, (case.index, value)
        for edge in case.edges[:4]:
            assert mdb.hist_cell_of(case.edges, edge) == np.searchsorted(qs.hist._keys(case.edges), qs.hist._keys(edge), side="right")
        checked += len(rows)
        # the whole-batch histogram holds every point inside the time range once
        t_lo, t_hi = qs._time_bounds(*case.time_range)
        assert int(expected.hist.sum()) == int(((case.timestamps >= t_lo) & (case.timestamps <= t_hi)).sum())
    assert checked > 500


def test_filter_bounds_sit_on_swing_points_for_each_of_the_four_searches(soak):
    """model_run finds the passing interval of a Swing segment with one binary search per end and direction; each of
    the four only matters when a bound equals a point inside a line that does not pass as a whole. At least two cases
    for each: a Swing segment with regular timestamps, rising or falling, with a point ON the closed lower (upper)
    bound and a point below (above) it."""
    met = {}
    for case, _ in soak:
        low, high = qs.bucket_filter._key_bounds(qs.value_filter(case))
        keys = qs.hist._keys(case.values)
        starts = np.concatenate([[0], np.cumsum(np.bincount(case.segment, minlength=len(case.batch)))])
        for row in np.flatnonzero(case.batch.model_type_id == mdb.MDB_SWING_ID):
            of_row = slice(starts[row], starts[row + 1])
            run, steps = keys[of_row], np.diff(case.timestamps[of_row])
            if len(run) < 3 or not (steps == steps[0]).all() or case.batch.residuals.lengths()[row] != 0:
                continue
            direction = "rising" if run[0] <= run[-1] else "falling"
            if (run == low).any() and (run < low).any():
                met.setdefault((direction, "lower"), set()).add(case.index)
            if (run == high).any() and (run > high).any():
                met.setdefault((direction, "upper"), set()).add(case.index)
    print({name: sorted(found) for name, found in met.items()})
    for name in (("rising", "lower"), ("rising", "upper"), ("falling", "lower"), ("falling", "upper")):
        assert len(met.get(name, ())) >= 2, (name, met)
