"""Plans and composed references of the shard soak (a helper module: tests/test_gpu_shard_soak.py runs the plans on
the GPU, tests/test_shard_soak_cpu.py keeps this file honest).

DESIGN.md section 6 scales the library past one GPU by giving every rank a contiguous block of series: a rank runs the
operators on its own segments and the partial results are folded on the host. plan(index) takes
tests/linked_soak.py's case `index` (tests/query_soak.py's hostile domain under three groupings, with tails of
single-point segments) and cuts the batch's segment rows into 2 to 6 contiguous shards, twice:

  seams      cuts only where the linked operators have no link under ANY max_gap: the last row before the cut and the
             first row after it differ in group, or time does not move forward. Episodes continue on "time not stepping
             back" and look only at the rows inside the filter's time range, so they have a seam set of their own
             (`episode_cuts`). A batch in series order (not permuted, grouped by series) is cut into the rank blocks of
             sharding.series_range for a world of 2, 3, n_series or n_series + 2: the last gives ranks with no series.
             Where two groups meet at a seam, one cut lies between groups. A case without a seam gets one empty shard
             and the whole batch.
  anywhere   cuts uniform over 0 .. len(batch), repeats allowed (empty shards, the first and the last included); one cut
             is forced onto a boundary that severs a forward same-group link where the case has one, and one directly
             in front of or behind a single-point tail segment where the case has a tail.

sample_at gets one request more than the drawn case's where a row holds -0.0: instants through that row ("signed_zero"),
so that the "one contribution, bit for bit" promise of mdb_sample_merge_n is met by a value that 0.0 + x changes.

Shards are contiguous on purpose: a group's segments taken out of a permuted batch would make rows consecutive that
were not, and create links the one call does not have. A shard is batch.slice(a, b) with groups[a:b]: n_groups and the
group ids stay global.

The composed references are the operators' own, evaluated shard by shard and combined exactly: the linked intervals
of every shard's rows concatenated (integral, change, dwell), sample_cases.sample_rows per shard with the counts and the
Fractions added, episodes_cases.reference per shard with first_row / first_segment shifted. The unlinked operators'
cells depend on the set of their points only: their reference is query_soak.reference / trend_soak.reference of the
whole case under either plan. One kind of trend request is left out (trend_request_kept): trend_soak.reference takes x
as exact integers, which the operator promises below 2^53 only and keeps beyond it inside a run. A request that puts x
at 2^53 or beyond (a far one: x near 2^63, one ulp 2 048 microseconds) can put rows of different runs closer than one
ulp into one cell - under one group, a group per segment or a tail, or between the segments of a series sampled every
microsecond - and there the ONE call misses that reference as well (indices 41, 208 and 394).
tests/test_gpu_trend_soak.py keeps such requests, in one call on its own 200 cases. Under `seams` every composed reference equals the whole-case one exactly. No arithmetic and no tolerance is defined here, and nothing here calls the library under test
apart from slicing batches the way linked_soak.slices does."""

import pickle
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import change_cases as chc
import dwell_cases as dc
import episodes_cases as ec
import integral_cases as ic
import linked_soak as ls
import query_soak as qs
import sample_cases as sc
import trend_soak as tts
from modelardb_rs_amd import sharding

SEED = 0x53485244
PLANS = ("seams", "anywhere")
MAX_CUTS = 5   # 2 to 6 shards
I64_MIN, I64_MAX = qs.I64_MIN, qs.I64_MAX


# ---- the plans -------------------------------------------------------------------------------------------------------

def _boundary_rows(drawn, starts, inside=None):
    """Per segment boundary b = 1 .. len(batch) - 1: (the last row before it, the first row after it), -1 where there is
    none; with `inside`, among the rows it marks."""
    n = len(drawn.batch)
    if inside is None:
        return starts[1:n] - 1, starts[1:n].copy()
    rows = np.flatnonzero(inside)
    if len(rows) == 0:
        return np.full(n - 1, -1), np.full(n - 1, -1)
    at = np.searchsorted(rows, starts[1:n])
    return (np.where(at > 0, rows[np.maximum(at - 1, 0)], -1),
            np.where(at < len(rows), rows[np.minimum(at, len(rows) - 1)], -1))


def _seams(drawn, starts):
    """(linked seams, episode seams, link boundaries): the boundaries 1 .. len(batch) - 1 over which the linked
    operators have no link under any max_gap, over which no episode continues, and over which a forward same-group link
    runs."""
    t, g = drawn.timestamps, drawn.row_groups
    boundaries = np.arange(1, len(drawn.batch))
    p, q = _boundary_rows(drawn, starts)
    same = g[p] == g[q]
    linked = boundaries[~same | (t[q] <= t[p])]
    links = boundaries[same & (t[q] > t[p])]
    t_lo, t_hi = drawn.filter_spec.get("t_lo", I64_MIN), drawn.filter_spec.get("t_hi", I64_MAX)
    p, q = _boundary_rows(drawn, starts, (t >= t_lo) & (t <= t_hi))
    continues = (p >= 0) & (q >= 0) & (g[p] == g[q]) & (t[q] >= t[p])
    return linked, boundaries[~continues], links


def _pick(rng, pool, n_cuts):
    return sorted(int(c) for c in rng.choice(pool, size=min(n_cuts, len(pool)), replace=False))


def _seams_plan(rng, drawn, starts, linked, episode_seams):
    n = len(drawn.batch)
    n_series = len(drawn.kinds)
    if not drawn.permuted and drawn.grouping == "series":
        # the rank blocks of DESIGN section 6; a tail lies behind the last series and goes with it
        worlds = sorted({2, 3, n_series, n_series + 2} - {1})
        world = int(worlds[int(rng.integers(0, len(worlds)))])
        first_segment = np.searchsorted(drawn.series_of_segment[:n - drawn.n_tail], np.arange(n_series))
        first_segment = np.concatenate([first_segment, [n]])
        cuts = [int(first_segment[sharding.series_range(n_series, rank, world)[0]]) for rank in range(1, world)]
        return SimpleNamespace(name="seams", cuts=cuts, episode_cuts=list(cuts), world=world)
    n_cuts = int(rng.integers(1, MAX_CUTS + 1))
    nothing = [[0], [n]][int(rng.integers(0, 2))]
    cuts = _pick(rng, linked, n_cuts) if len(linked) else nothing
    group_of_segment = drawn.row_groups[starts[:-1]]
    between = [int(c) for c in linked if group_of_segment[c - 1] != group_of_segment[c]]
    if between and not set(between) & set(cuts):   # where two groups meet, one cut lies between groups
        cuts[int(rng.integers(0, len(cuts)))] = between[int(rng.integers(0, len(between)))]
        cuts.sort()
    kept = [c for c in cuts if c in set(episode_seams.tolist())]
    episode_cuts = kept if kept else (_pick(rng, episode_seams, n_cuts) if len(episode_seams) else nothing)
    return SimpleNamespace(name="seams", cuts=cuts, episode_cuts=episode_cuts, world=None)


def _anywhere_plan(rng, drawn, links):
    n = len(drawn.batch)
    forced = []
    if len(links):
        forced.append(int(links[int(rng.integers(0, len(links)))]))
    if drawn.n_tail:
        segment = n - drawn.n_tail + int(rng.integers(0, drawn.n_tail))
        forced.append(segment + int(rng.integers(0, 2)))   # in front of it or behind it
    n_cuts = max(int(rng.integers(1, MAX_CUTS + 1)), len(forced))
    cuts = sorted(forced + [int(c) for c in rng.integers(0, n + 1, n_cuts - len(forced))])
    return SimpleNamespace(name="anywhere", cuts=cuts, episode_cuts=list(cuts), world=None)


def _signed_zero_request(rng, drawn):
    """One more request for sample_at where a row holds -0.0: instants through that row. A cell whose one contribution
    is that row must hold -0.0 through the fold, which 0.0 + x does not give: the default indices' own_grid requests
    hold no such cell."""
    rows = np.flatnonzero(drawn.values.view(np.uint32) == 0x80000000)
    if len(rows) == 0:
        return None
    at = int(drawn.timestamps[int(rows[int(rng.integers(0, len(rows)))])])
    steps = np.diff(drawn.timestamps)
    steps = steps[steps > 0]
    width = int([1, int(np.median(steps)) if len(steps) else 1][int(rng.integers(0, 2))])
    n_instants = min(qs.MAX_CELLS // drawn.n_groups, int([1, 16, 256][int(rng.integers(0, 3))]))
    return SimpleNamespace(style="signed_zero", origin=at - int(rng.integers(0, n_instants)) * width, width=width,
                           n_buckets=n_instants, max_gap=None, gap_choice="none")


def plan(index):
    """Everything the shard soak of case `index` needs, a pure function of `index`; None where linked_soak.draw leaves
    the case out. `drawn` is linked_soak's case, `whole` the same batch in the shape query_soak.reference takes (the
    unlinked operators'), `trend_requests` what trend_soak.draw gives for the index, `sample_requests`
    the drawn case's and the signed-zero one, `plans` the two plans by name."""
    drawn = ls.draw(index)
    if drawn is None:
        return None
    case, trend_requests = tts.draw(index)
    rng = np.random.default_rng([SEED, index])
    n = len(drawn.batch)
    rows = np.bincount(drawn.segment, minlength=n)
    assert (rows > 0).all()
    starts = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    linked, episode_seams, links = _seams(drawn, starts)
    plans = {"seams": _seams_plan(rng, drawn, starts, linked, episode_seams),
             "anywhere": _anywhere_plan(rng, drawn, links)}
    link_set = set(links.tolist())
    for one in plans.values():
        assert 1 <= len(one.cuts) <= MAX_CUTS and 1 <= len(one.episode_cuts) <= MAX_CUTS
        assert all(0 <= a <= b <= n for a, b in zip([0] + one.cuts, one.cuts + [n]))
        one.severed = sorted({c for c in one.cuts if c in link_set})
    assert not plans["seams"].severed
    whole = SimpleNamespace(index=index, batch=drawn.batch, n_groups=drawn.n_groups, timestamps=drawn.timestamps,
                            groups=np.zeros(n, dtype=np.uint32) if drawn.groups is None else drawn.groups,
                            values=drawn.values, segment=drawn.segment, requests=case.requests,
                            filter_spec=drawn.filter_spec, edges=case.edges, q=case.q, time_range=case.time_range,
                            slice_pairs=case.slice_pairs)
    signed_zero = _signed_zero_request(rng, drawn)   # (drawn after the plans: they do not depend on it)
    return SimpleNamespace(index=index, drawn=drawn, whole=whole, trend_requests=trend_requests, linked={},
                           sample_requests=drawn.sample_requests + ([] if signed_zero is None else [signed_zero]),
                           edges=case.edges, plans=plans, starts=starts, rows_of_segment=rows, links=links,
                           linked_seams=linked, episode_seams=episode_seams)


def plan_bytes(planned):
    """Everything plan() decided, as bytes."""
    plans = [(one.name, one.cuts, one.episode_cuts, one.world, one.severed) for one in planned.plans.values()]
    requests = [tuple(sorted(vars(request).items())) for request in planned.trend_requests + planned.sample_requests]
    return pickle.dumps((ls.case_bytes(planned.drawn), planned.edges.tobytes(), requests, plans))


def bounds(planned, cuts):
    """[(first segment row, one past the last)] of the shards of a list of cuts."""
    return list(zip([0] + list(cuts), list(cuts) + [len(planned.drawn.batch)]))


def shards(planned, cuts):
    """([batch per shard], [groups per shard], or None where the case has one group)."""
    drawn = planned.drawn
    return ([drawn.batch.slice(a, b) for a, b in bounds(planned, cuts)],
            None if drawn.groups is None else [drawn.groups[a:b] for a, b in bounds(planned, cuts)])


def trend_request_kept(planned, request):
    """Does trend_soak.reference hold for the request however the rows are cut into runs and calls? Where every
    x = (t - origin) - bucket * width lies below 2^53, where the operator's x is exact (mdb.h). Beyond that - a far
    request - x is rounded to its ulp wherever two runs meet, and the reference's exact integers are more than the
    contract gives: the one call meets them only while the runs of a cell lie further apart than that."""
    inside, cells = qs.place(planned.whole, request)
    buckets = cells % request.n_buckets
    return all((int(t) - request.origin) - int(b) * request.width < 1 << 53
               for t, b in zip(planned.whole.timestamps[inside], buckets))


def describe(one):
    world = "" if one.world is None else f", the rank blocks of a world of {one.world}"
    return f"plan {one.name}: cuts {one.cuts} (episodes {one.episode_cuts}){world}, severed links at {one.severed}"


# ---- the references ----------------------------------------------------------------------------------------------------

def _row_ranges(planned, cuts):
    return [(int(planned.starts[a]), int(planned.starts[b])) for a, b in bounds(planned, cuts)]


def composed_linked(planned, one, max_gap):
    """integral_cases.linked_intervals of every shard's rows, concatenated; kept in planned.linked."""
    kept = planned.linked.setdefault(one.name, {})
    if max_gap not in kept:
        drawn, out = planned.drawn, []
        for r0, r1 in _row_ranges(planned, one.cuts):
            out += ic.linked_intervals(drawn.timestamps[r0:r1], drawn.values[r0:r1], drawn.row_groups[r0:r1], max_gap)
        kept[max_gap] = out
    return kept[max_gap]


def composed_integral(planned, one, request, method):
    return ic.cells_of(composed_linked(planned, one, request.max_gap), planned.drawn.n_groups, request.origin,
                       request.width, request.n_buckets, method)


def composed_change(planned, one, request):
    return chc.cells_of(composed_linked(planned, one, request.max_gap), planned.drawn.n_groups, request.origin,
                        request.width, request.n_buckets)


def composed_dwell(planned, one, request):
    return dc.cells_of(composed_linked(planned, one, request.max_gap), planned.edges, planned.drawn.n_groups,
                       request.origin, request.width, request.n_buckets)


def whole_dwell(planned, request):
    return dc.cells_of(ls.linked(planned.drawn, request.max_gap), planned.edges, planned.drawn.n_groups, request.origin,
                       request.width, request.n_buckets)


def composed_sample(planned, one, request, method):
    """sample_cases.sample_rows per shard: the counts added, the Fractions of sum and scale added, finite AND-ed (the
    sum of a cell that is not finite is 0, as sample_rows writes it)."""
    drawn, out = planned.drawn, None
    for r0, r1 in _row_ranges(planned, one.cuts):
        part = sc.sample_rows(drawn.timestamps[r0:r1], drawn.values[r0:r1], drawn.row_groups[r0:r1], drawn.n_groups,
                              request.origin, request.width, request.n_buckets, method, request.max_gap)
        if out is None:
            out = part
        else:
            out = {"count": out["count"] + part["count"], "sum": out["sum"] + part["sum"],
                   "scale": out["scale"] + part["scale"], "finite": out["finite"] & part["finite"]}
    out["sum"] = np.where(out["finite"], out["sum"], Fraction(0))
    return out


def composed_episodes(planned, one, rule):
    """episodes_cases.reference per shard of the plan's episode cuts, first_row and first_segment shifted by where the
    shard starts (first_row counts the rows inside the filter's time range, as n_rows does), the lists concatenated in
    shard order, n_rows and n_passing added: (episodes, magnitudes, n_rows, n_passing)."""
    drawn = planned.drawn
    flt = ls.value_filter(drawn)
    episodes, magnitudes, n_rows, n_passing = [], [], 0, 0
    for (a, b), (r0, r1) in zip(bounds(planned, one.episode_cuts), _row_ranges(planned, one.episode_cuts)):
        table = SimpleNamespace(batch=range(a, b), ts=drawn.timestamps[r0:r1], values=drawn.values[r0:r1],
                                segment=drawn.segment[r0:r1] - a)
        part, sums, rows, passing, _ = ec.reference(table, flt, None if drawn.groups is None else drawn.groups[a:b],
                                                    rule.max_gap, rule.min_duration, rule.min_count)
        episodes.append(shifted(part, n_rows, a))
        magnitudes.append(sums)
        n_rows, n_passing = n_rows + rows, n_passing + passing
    return np.concatenate(episodes), np.concatenate(magnitudes), n_rows, n_passing


def shifted(episodes, first_row, first_segment):
    """A shard's episodes numbered as the whole batch numbers them."""
    out = episodes.copy()
    out["first_row"] += np.uint64(first_row)
    out["first_segment"] += np.uint32(first_segment)
    return out


def same(a, b):
    """Are two references equal in every member (dicts of arrays, arrays, lists or tuples of them)? Floats by bit
    pattern, Fractions by value."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[name], b[name]) for name in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        if a.shape != b.shape or a.dtype != b.dtype:
            return False
        return bool((a == b).all()) if a.dtype == object else a.tobytes() == b.tobytes()
    return a == b


def severed_microseconds(planned, one, request, operator):
    """Per group, the microseconds the plan's severed links would have added to the durations of `operator`
    ("integral": the link clipped to the window; "change": the whole link where its later row lies in the window),
    from the two rows either side of every severed boundary."""
    drawn = planned.drawn
    out = [0] * drawn.n_groups
    last = request.origin + request.n_buckets * request.width
    for boundary in one.severed:
        q = int(planned.starts[boundary])
        t0, t1, group = int(drawn.timestamps[q - 1]), int(drawn.timestamps[q]), int(drawn.row_groups[q])
        assert t1 > t0 and group == int(drawn.row_groups[q - 1])
        if request.max_gap is not None and t1 - t0 > request.max_gap:
            continue
        if operator == "integral":
            out[group] += max(0, min(t1, last) - max(t0, request.origin))
        elif request.origin <= t1 < last:
            out[group] += t1 - t0
    return out


def duration_per_group(duration):
    """The durations of a (n_groups, n_buckets) result summed per group, as Python integers."""
    return [sum(int(x) for x in row) for row in duration]


# ---- the census: what a plan holds ---------------------------------------------------------------------------------------

def plan_census(planned, one):
    drawn = planned.drawn
    n = len(drawn.batch)
    single = planned.rows_of_segment == 1
    groups = np.zeros(n, dtype=np.int64) if drawn.groups is None else drawn.groups.astype(np.int64)
    shard_bounds = bounds(planned, one.cuts)
    filled = [(a, b) for a, b in shard_bounds if b > a]
    between_groups = [c for c in one.cuts if 0 < c < n and groups[c - 1] != groups[c]]
    return {"shards": len(shard_bounds),
            "empty shards": len(shard_bounds) - len(filled),
            "shards that begin or end with a single-point segment": sum(bool(single[a] or single[b - 1]) for a, b in filled),
            "shards without a row of some group": sum(len(set(groups[a:b].tolist())) < drawn.n_groups for a, b in filled),
            "cuts between groups": len(between_groups),
            "severed links": len(one.severed),
            "ranks without a series": 0 if one.world is None else max(0, one.world - len(drawn.kinds))}
