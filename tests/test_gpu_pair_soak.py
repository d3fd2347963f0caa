"""Randomised differential soak of the two operators that take two fields - comoments_buckets and binned_buckets -
over the cases of tests/pair_soak.py: the hostile input domain of tests/test_gpu_soak.py in an x field (permuted in
half the cases, under three groupings) against a y field compressed on its own, of six kinds (independent, with NaN
and infinities where x has none, constant, the negative of x, x itself, single-point segments), with tails of
single-point segments, time ranges that cut segments, buckets far below the data, a microsecond wide and dense, edges
on the points of Swing lines, list cuts that differ per field and slices of 1 to 1 000 runs.

One-call tier: every request runs through the host form, twice through the dev form on one upload per field and, where
the case has list cuts, through the list form; all give the same bytes. The host form is held to the operator's own
reference under the operator's own rule (comoments_cases / binned_cases.assert_cells: no tolerance is set here); a cell
that the f64 emulation of the documented rule (pair_soak.rule_cells / rule_binned) cannot bring within that tolerance
is held to its exact members only - count, finiteness, m2 >= 0. The counts are those of agg_buckets and hist_buckets of
x; binned's cells folded over the value cells give comoments' y moments; the laws of the y kinds, the swap of the two
fields and the slice sizes follow.

Shard tier: both fields cut at the same series boundaries (or at a common cut row inside a series) into calls whose
cells are folded with comoments_merge / moments_merge in both orders and chained through inout: counts and empty cells
have the one call's bytes, the f64 members meet the REFERENCE. A cut that leaves the fields with different row counts
is refused.

MDB_PAIR_SOAK_CASES sets the number of indices (default 60; an index whose case has more than 8 192 rows is left out);
the long run is recorded in MEASUREMENTS.md. Every case is a pure function of its index:
scripts/debug_pair_soak_case.py INDEX [one|shards] replays one."""

import os
import re

import numpy as np
import pytest

import binned_cases as bc
import comoments_cases as cc
import linked_soak as ls
import pair_soak as ps
import query_soak as qs
import modelardb_rs_amd as mdb
from test_gpu_linked_soak import PAIRS_SWITCH, _option

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("MDB_PAIR_SOAK_CASES", "60"))
BLOCK = 10  # indices per pytest item (halved from 20; see DESIGN.md section 2 for the slowest item)
BLOCKS = range((N_CASES + BLOCK - 1) // BLOCK)
SHARD_CASES, SHARD_BLOCK = 30, 10
SHARD_BLOCKS = range(SHARD_CASES // SHARD_BLOCK)
CO, MO = mdb.COMOMENTS_CELL_DTYPE, mdb.MOMENTS_CELL_DTYPE


class _Census:
    def __init__(self):
        self.cases = self.requests = self.runs = self.comparisons = 0
        self.cells = {"comoments": 0, "binned": 0}
        self.ill = {"comoments": 0, "binned": 0}
        self.special = {"comoments": 0, "binned": 0}
        self.worst = {}

    def add(self, operator, got, expected, well, plain):
        self.comparisons += 1
        self.cells[operator] += int(plain.sum())
        self.ill[operator] += int((plain & ~well).sum())
        self.special[operator] += int(((expected["count"] > 0) & ~plain).sum())
        for name, ratio in ps.worst_ratios(got, expected, well, plain, binned=operator == "binned").items():
            key = f"{operator} {name}"
            self.worst[key] = max(self.worst.get(key, 0.0), ratio)

    def tell(self, title):
        worst = ", ".join(f"{name} {ratio:.3g}" for name, ratio in sorted(self.worst.items()))
        print(f"{title}: {self.cases} cases, {self.requests} requests, {self.comparisons} comparisons, "
              f"{self.cells['comoments']} comoments cells and {self.cells['binned']} binned cells of finite points "
              f"({self.ill['comoments']} and {self.ill['binned']} of them ill-conditioned), {self.special['comoments']} and "
              f"{self.special['binned']} with a non-finite point, {self.runs} binned runs; worst error / allowed: {worst}")


def _uploaded(hip, drawn):
    dev_x = hip.upload_segments(drawn.x.batch)
    return dev_x, dev_x if drawn.y is drawn.x else hip.upload_segments(drawn.y.batch)


def _free(dev_x, dev_y):
    dev_x.free()
    if dev_y is not dev_x:
        dev_y.free()


def _comoments_forms(hip, drawn, dev, request):
    args, ranged = ps.window(request)
    common = dict(ranged, n_groups=drawn.n_groups)
    out = [("host", hip.comoments_buckets(drawn.x.batch, drawn.y.batch, *args, groups=drawn.groups, **common)),
           ("dev", hip.comoments_buckets_dev(*dev, *args, groups=drawn.groups, **common)),
           ("dev again", hip.comoments_buckets_dev(*dev, *args, groups=drawn.groups, **common))]
    if drawn.x_cuts is not None:
        xs, ys, groups = ps.slices(drawn)
        out.append(("list", hip.comoments_buckets_list(xs, ys, *args, groups=groups, **common)))
    return out


def _binned_forms(hip, drawn, dev, request):
    args, ranged = ps.window(request)
    common = dict(ranged, n_groups=drawn.n_groups)
    out = [("host", hip.binned_buckets(drawn.x.batch, drawn.y.batch, drawn.edges, *args, groups=drawn.groups, **common)),
           ("dev", hip.binned_buckets_dev(*dev, drawn.edges, *args, groups=drawn.groups, **common)),
           ("dev again", hip.binned_buckets_dev(*dev, drawn.edges, *args, groups=drawn.groups, **common))]
    if drawn.x_cuts is not None:
        xs, ys, groups = ps.slices(drawn)
        out.append(("list", hip.binned_buckets_list(xs, ys, drawn.edges, *args, groups=groups, **common)))
    return out


def _same_bytes(forms):
    return [f"the {form} form differs from the host form's bytes" for form, result in forms[1:]
            if result.tobytes() != forms[0][1].tobytes()]


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _laws(drawn, co, bi, expected_co, expected_bi, well, plain):
    """The laws of the y kinds in cells of finite points (mdb.h: the merge rule of mdb_comoments_buckets)."""
    out = []
    if drawn.kind == "self":
        if not (_same(co["m2_x"][plain], co["m2_y"][plain]) and _same(co["m2_x"][plain], co["c_xy"][plain])):
            out.append("self: m2_x, m2_y and c_xy differ in their bytes")
        if not _same(co["mean_x"][plain], co["mean_y"][plain]):
            out.append("self: mean_x and mean_y differ in their bytes")
    elif drawn.kind == "constant":
        flat = plain & (expected_co["m2_y"] == 0.0)   # (the cells in which y IS constant: not where series or a tail meet)
        if not ((co["c_xy"][flat] == 0.0).all() and (co["m2_y"][flat] == 0.0).all()):
            out.append("constant: c_xy or m2_y is not 0.0 in a cell of one y value")
        if not _same(co["mean_y"][flat], expected_co["mean_y"][flat]):
            out.append("constant: mean_y is not the value")
        flat = (expected_bi["count"] > 0) & expected_bi["finite"] & (expected_bi["m2"] == 0.0)
        if not ((bi["m2"][flat] == 0.0).all() and _same(bi["mean"][flat], expected_bi["mean"][flat])):
            out.append("constant: binned m2 is not 0.0 or mean is not the value in a cell of one y value")
    elif drawn.kind == "negated" and not drawn.permuted:
        # (a mean of zero has no sign to negate: K + s / n with s == +0.0 is +0.0 for x = 0.0 and for y = -0.0 alike -
        # DESIGN.md section 7, pinned by tests/test_pair_soak_cpu.py)
        zero = (co["mean_x"] == 0.0) & (co["mean_y"] == 0.0)
        if not _same(co["mean_y"][plain & ~zero], -co["mean_x"][plain & ~zero]):
            out.append("negated: mean_y has not the bytes of -mean_x")
        if not _same(co["m2_y"][plain], co["m2_x"][plain]):
            out.append("negated: m2_y has not the bytes of m2_x")
        if not (co["c_xy"][plain] <= 0.0).all():
            out.append("negated: c_xy > 0")
        if not (np.abs(co["c_xy"] + co["m2_x"])[plain & well] <= cc.C_TOLERANCE * co["m2_x"][plain & well]).all():
            out.append("negated: c_xy is not -m2_x within the tolerance")
    return out


def _fold_differences(bi, expected_co, well_co, well_bi):
    """binned's cells of a (group, bucket) folded over the value cells against comoments' y moments (the reference's)."""
    folded = ps.folded_binned(bi)
    keep = (expected_co["count"] > 0) & expected_co["finite_x"] & expected_co["finite_y"] & well_co & well_bi.all(axis=2)
    out = []
    if not np.array_equal(folded["count"], expected_co["count"]):
        out.append("binned folded over the value cells: count differs from comoments'")
    with np.errstate(invalid="ignore"):
        if not (np.abs(folded["mean"] - expected_co["mean_y"])[keep] <= bc.MEAN_TOLERANCE * expected_co["largest_y"][keep]).all():
            out.append("binned folded over the value cells: mean misses comoments' mean_y")
        if not (np.abs(folded["m2"] - expected_co["m2_y"])[keep] <= bc.M2_TOLERANCE * expected_co["m2_y"][keep]).all():
            out.append("binned folded over the value cells: m2 misses comoments' m2_y")
    return out


def _one_call(hip, drawn, dev, census, tell):
    for request in drawn.requests:
        census.requests += 1
        args, ranged = ps.window(request)
        common = dict(ranged, n_groups=drawn.n_groups)
        # comoments
        forms = _comoments_forms(hip, drawn, dev, request)
        co = forms[0][1]
        expected_co = ps.reference_comoments(drawn, request)
        well_co, plain_co = ps.well_conditioned_cells(ps.rule_cells(drawn, request), expected_co)
        tell(request, "comoments", _same_bytes(forms) + ps.comoments_differences(co, expected_co, well_co, plain_co))
        census.add("comoments", co, expected_co, well_co, plain_co)
        counted = hip.agg_buckets(drawn.x.batch, *args, groups=drawn.groups, which_mask=mdb.MDB_AGG_COUNT, **common)
        tell(request, "comoments against agg_buckets", qs.exact_differences(co["count"], counted["count"], "count"))
        # binned
        forms = _binned_forms(hip, drawn, dev, request)
        bi = forms[0][1]
        expected_bi = ps.reference_binned(drawn, request)
        well_bi, plain_bi = ps.well_conditioned_binned(ps.rule_binned(drawn, request), expected_bi)
        tell(request, "binned", _same_bytes(forms) + ps.binned_differences(bi, expected_bi, well_bi, plain_bi))
        census.add("binned", bi, expected_bi, well_bi, plain_bi)
        census.runs += expected_bi["runs"]
        counted = hip.hist_buckets(drawn.x.batch, drawn.edges, *args, groups=drawn.groups, **common)
        tell(request, "binned against hist_buckets",
             qs.exact_differences(bi["count"], np.asarray(counted).astype(np.int64), "count"))
        tell(request, "binned against comoments", _fold_differences(bi, expected_co, well_co, well_bi))
        tell(request, f"the laws of a {drawn.kind} y", _laws(drawn, co, bi, expected_co, expected_bi, well_co, plain_co))
        # the two fields exchanged: the same pairs, in the bucket of the same instant and the group of the same series
        if not drawn.permuted and drawn.grouping == "series":
            groups = ps.y_groups(drawn)
            swapped = hip.comoments_buckets(drawn.y.batch, drawn.x.batch, *args, groups=groups, **common)
            expected = ps.reference_comoments(drawn, request, swapped=True)
            well, plain = ps.well_conditioned_cells(ps.rule_cells(drawn, request, swapped=True), expected)
            differences = ps.comoments_differences(swapped, expected, well, plain)
            differences += qs.exact_differences(swapped["count"], co["count"], "count of the swapped call")
            for ours, theirs in (("mean_x", "mean_y"), ("mean_y", "mean_x"), ("c_xy", "c_xy")):   # (the references agree)
                if not np.array_equal(expected[ours], expected_co[theirs]):
                    differences.append(f"the swapped reference's {ours} is not the reference's {theirs}")
            tell(request, "comoments(y, x)", differences)
            census.add("comoments", swapped, expected, well, plain)
        # the slice sizes: the order of the merges changes, the counts do not
        if drawn.slice_pairs is not None:
            for size in ls.SLICE_PAIRS:
                with _option(hip, PAIRS_SWITCH, size):
                    sliced_co = hip.comoments_buckets(drawn.x.batch, drawn.y.batch, *args, groups=drawn.groups, **common)
                    sliced_bi = hip.binned_buckets(drawn.x.batch, drawn.y.batch, drawn.edges, *args, groups=drawn.groups,
                                                   **common)
                differences = qs.exact_differences(sliced_co["count"], co["count"], "comoments count")
                differences += qs.exact_differences(sliced_bi["count"], bi["count"], "binned count")
                differences += ps.comoments_differences(sliced_co, expected_co, well_co, plain_co)
                differences += ps.binned_differences(sliced_bi, expected_bi, well_bi, plain_bi)
                tell(request, f"slices of {size}", differences)
                census.add("comoments", sliced_co, expected_co, well_co, plain_co)
                census.add("binned", sliced_bi, expected_bi, well_bi, plain_bi)


def _teller(drawn, tier, report=None):
    def tell(request, what, differences):
        where = f"pair soak case {drawn.index} ({tier}; y {drawn.kind}, {drawn.grouping}, tail {drawn.n_tail}, " \
                f"{'permuted' if drawn.permuted else 'in order'}), {ps.describe(request)}"
        if report is not None:
            report(where, what, differences)
        else:
            assert not differences, (where, what, differences[:5])
    return tell


def run_case(hip, index, census, report=None):
    """One case through the one-call tier. Returns the drawn case, None when it is left out for its size."""
    drawn = ps.draw(index)
    if drawn is None:
        return None
    dev = _uploaded(hip, drawn)
    try:
        _one_call(hip, drawn, dev, census, _teller(drawn, "one call", report))
    finally:
        _free(*dev)
        qs.forget_grids()
    census.cases += 1
    return drawn


def _pattern(shape, dtype):
    """Cells prefilled with bytes no call writes."""
    return np.frombuffer(bytes((7 * k + 3) % 251 for k in range(int(np.prod(shape)) * dtype.itemsize)),
                         dtype=dtype).reshape(shape).copy()


def _refused(hip, drawn, x_batch, y_batch, groups, request):
    """Both operators in both forms on fields whose row counts differ: refused, the message names both counts, inout
    keeps its bytes. Returns the differences."""
    args, ranged = ps.window(request)
    common = dict(ranged, n_groups=drawn.n_groups, groups=groups)
    t_lo, t_hi = ps.time_bounds(request)
    n_x = int(ps.Field(x_batch).in_range(t_lo, t_hi).sum()) if len(x_batch) else 0
    n_y = int(ps.Field(y_batch).in_range(t_lo, t_hi).sum()) if len(y_batch) else 0
    assert n_x != n_y
    out = []
    dev_x, dev_y = hip.upload_segments(x_batch), hip.upload_segments(y_batch)
    try:
        co, bi = _pattern((drawn.n_groups, request.n_buckets), CO), \
            _pattern((drawn.n_groups, request.n_buckets, len(drawn.edges) + 1), MO)
        calls = [("comoments host", co, lambda: hip.comoments_buckets(x_batch, y_batch, *args, cells=co, **common)),
                 ("comoments dev", co, lambda: hip.comoments_buckets_dev(dev_x, dev_y, *args, cells=co, **common)),
                 ("binned host", bi, lambda: hip.binned_buckets(x_batch, y_batch, drawn.edges, *args, cells=bi, **common)),
                 ("binned dev", bi, lambda: hip.binned_buckets_dev(dev_x, dev_y, drawn.edges, *args, cells=bi, **common))]
        for name, cells, call in calls:
            before = cells.tobytes()
            try:
                call()
                out.append(f"{name}: {n_x} rows of x against {n_y} rows of y were not refused")
            except mdb.HipError as error:
                if not re.search(rf"\b{n_x} rows.*\b{n_y} rows", str(error)):
                    out.append(f"{name}: the message does not name {n_x} and {n_y}: {error}")
            if cells.tobytes() != before:
                out.append(f"{name}: inout changed")
    finally:
        dev_x.free()
        dev_y.free()
    return out


def _refused_without_the_last_segment(hip, drawn):
    """y given without its last segment, under the first request whose range reaches that segment's rows."""
    y = drawn.y
    first_missing = y.ts[y.starts[len(y.batch) - 1]:]
    for request in drawn.requests:
        t_lo, t_hi = ps.time_bounds(request)
        if ((first_missing >= t_lo) & (first_missing <= t_hi)).any():
            differences = _refused(hip, drawn, drawn.x.batch, y.batch.slice(0, len(y.batch) - 1), drawn.groups, request)
            _teller(drawn, "refused call")(request, "y without its last segment", differences)
            return True
    return False


@pytest.mark.parametrize("block", BLOCKS)
def test_one_call(hip, block):
    census = _Census()
    indices = range(block * BLOCK, min(N_CASES, (block + 1) * BLOCK))
    refused = False
    for index in indices:
        drawn = run_case(hip, index, census)
        if drawn is not None and not refused and len(drawn.y.batch) >= 2:
            refused = _refused_without_the_last_segment(hip, drawn)   # (once per item)
    census.tell(f"one call, indices {indices[0]} to {indices[-1]}")
    assert 2 * census.cases >= len(indices) and refused
    assert census.cells["comoments"] > 0 and census.cells["binned"] > 0


# ---- the shard tier ------------------------------------------------------------------------------------------------------

def _shard_bounds(cuts, n):
    return list(zip([0] + list(cuts), list(cuts) + [n]))


def _series_seams(drawn):
    """(x cuts, y cuts): both fields cut at the same series boundaries into 2 to 4 shards, each field's segment indices
    from its own series array; a tail goes with the last series. One series: the whole batch and an empty shard."""
    rng = np.random.default_rng([ps.SEED, drawn.index, 1])
    if drawn.n_series == 1:
        return [len(drawn.x.batch)], [len(drawn.y.batch)]
    n_cuts = int(rng.integers(1, min(3, drawn.n_series - 1) + 1))
    series = np.sort(rng.choice(np.arange(1, drawn.n_series), size=n_cuts, replace=False))
    body_x, body_y = len(drawn.x.batch) - drawn.n_tail, len(drawn.y.batch) - drawn.n_tail
    return ([int(c) for c in np.searchsorted(drawn.x_series[:body_x], series)],
            [int(c) for c in np.searchsorted(drawn.y_series[:body_y], series)])


def _common_row_seam(drawn):
    """(x cut, y cut) at the common cut row of one series, None where no series has two rows."""
    rng = np.random.default_rng([ps.SEED, drawn.index, 2])
    rows = [row for row in drawn.common_rows if row is not None]
    if not rows:
        return None
    row = rows[int(rng.integers(0, len(rows)))]
    x_cut, y_cut = int(np.searchsorted(drawn.x.starts, row)), int(np.searchsorted(drawn.y.starts, row))
    assert drawn.x.starts[x_cut] == row and drawn.y.starts[y_cut] == row
    return x_cut, y_cut


def _shard_calls(hip, drawn, request, x_cuts, y_cuts, operator, tell):
    """(cells per shard from fresh cells, cells chained through inout) of one operator; the dev form on resident shards
    is held to the host form's bytes."""
    args, ranged = ps.window(request)
    common = dict(ranged, n_groups=drawn.n_groups)
    shape = (drawn.n_groups, request.n_buckets) + ((len(drawn.edges) + 1,) if operator == "binned" else ())
    parts = []
    chained = np.zeros(shape, dtype=MO if operator == "binned" else CO)
    shards = list(zip(_shard_bounds(x_cuts, len(drawn.x.batch)), _shard_bounds(y_cuts, len(drawn.y.batch))))
    for (xa, xb), (ya, yb) in shards:
        x_batch, y_batch = drawn.x.batch.slice(xa, xb), drawn.y.batch.slice(ya, yb)
        groups = None if drawn.groups is None else drawn.groups[xa:xb]
        if operator == "binned":
            host = lambda cells=None: hip.binned_buckets(x_batch, y_batch, drawn.edges, *args, groups=groups, cells=cells, **common)
            resident = lambda a, b: hip.binned_buckets_dev(a, b, drawn.edges, *args, groups=groups, **common)
        else:
            host = lambda cells=None: hip.comoments_buckets(x_batch, y_batch, *args, groups=groups, cells=cells, **common)
            resident = lambda a, b: hip.comoments_buckets_dev(a, b, *args, groups=groups, **common)
        part = host()
        chained = host(chained)
        if xb > xa and yb > ya:
            dev_x, dev_y = hip.upload_segments(x_batch), hip.upload_segments(y_batch)
            try:
                if resident(dev_x, dev_y).tobytes() != part.tobytes():
                    tell(request, operator, [f"shard x[{xa}:{xb}] y[{ya}:{yb}]: the dev form differs from the host form's bytes"])
            finally:
                dev_x.free()
                dev_y.free()
        parts.append(part)
    return parts, chained


def _folded(parts, merge):
    out = np.zeros_like(parts[0])
    for part in parts:
        merge(out.reshape(-1), part.reshape(-1))
    return out


def _sharded(hip, drawn, census, tell, x_cuts, y_cuts, name):
    for request in drawn.requests:
        census.requests += 1
        args, ranged = ps.window(request)
        common = dict(ranged, n_groups=drawn.n_groups)
        for operator, merge in (("comoments", mdb.comoments_merge), ("binned", mdb.moments_merge)):
            if operator == "comoments":
                whole = hip.comoments_buckets(drawn.x.batch, drawn.y.batch, *args, groups=drawn.groups, **common)
                expected = ps.reference_comoments(drawn, request)
                well, plain = ps.well_conditioned_cells(ps.rule_cells(drawn, request), expected)
                held = ps.comoments_differences
            else:
                whole = hip.binned_buckets(drawn.x.batch, drawn.y.batch, drawn.edges, *args, groups=drawn.groups, **common)
                expected = ps.reference_binned(drawn, request)
                well, plain = ps.well_conditioned_binned(ps.rule_binned(drawn, request), expected)
                held = ps.binned_differences
            parts, chained = _shard_calls(hip, drawn, request, x_cuts, y_cuts, operator, tell)
            empty = whole["count"] == 0
            for how, got in (("folded in order", _folded(parts, merge)), ("folded in reverse", _folded(parts[::-1], merge)),
                             ("chained through inout", chained)):
                differences = qs.exact_differences(got["count"], whole["count"], "count")
                if got[empty].tobytes() != whole[empty].tobytes():
                    differences.append("an empty cell has not the one call's bytes")
                differences += held(got, expected, well, plain)   # (the reference, not the one call)
                tell(request, f"{operator}, {name}, {how}", differences)
                census.add(operator, got, expected, well, plain)


def run_shard_case(hip, index, census, report=None):
    drawn = ps.draw(index)
    if drawn is None or drawn.permuted:
        return None
    tell = _teller(drawn, "shards", report)
    try:
        x_cuts, y_cuts = _series_seams(drawn)
        _sharded(hip, drawn, census, tell, x_cuts, y_cuts, f"series seams x{x_cuts} y{y_cuts}")
        seam = _common_row_seam(drawn)
        if seam is not None:
            x_cut, y_cut = seam
            _sharded(hip, drawn, census, tell, [x_cut], [y_cut], f"a seam inside a series x[{x_cut}] y[{y_cut}]")
            # x cut there alone, y one segment later: the first call's row counts differ
            request = next(r for r in drawn.requests if r.t_lo is None and r.t_hi is None)
            groups = None if drawn.groups is None else drawn.groups[:x_cut]
            differences = _refused(hip, drawn, drawn.x.batch.slice(0, x_cut), drawn.y.batch.slice(0, y_cut + 1), groups, request)
            tell(request, f"the uneven cut x[:{x_cut}] y[:{y_cut + 1}]", differences)
            census.refused = getattr(census, "refused", 0) + 1
    finally:
        qs.forget_grids()
    census.cases += 1
    return drawn


def shard_indices():
    """The default indices whose x is in series order, at most SHARD_CASES of them."""
    return [index for index in range(min(N_CASES, 60)) if (lambda d: d is not None and not d.permuted)(ps.draw(index))][:SHARD_CASES]


@pytest.mark.parametrize("block", SHARD_BLOCKS)
def test_shards(hip, block):
    census = _Census()
    indices = shard_indices()[block * SHARD_BLOCK:(block + 1) * SHARD_BLOCK]
    for index in indices:
        run_shard_case(hip, index, census)
    census.tell(f"shards, indices {indices}")
    if indices:
        assert census.cases == len(indices) and getattr(census, "refused", 0) > 0
        assert census.cells["comoments"] > 0 and census.cells["binned"] > 0


def test_cases_that_once_failed(hip):
    for index, tier in ():
        (run_case if tier == "one call" else run_shard_case)(hip, index, _Census())
