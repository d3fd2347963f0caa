"""Layout invariance: a batch's results do not depend on where its payload bytes lie.

Every operator family is handed the corpus of tests/layouts.py in six physical layouts of its BinaryView columns (one
padded buffer with shuffled payloads, three buffers, an empty first buffer, arrow's growing blocks, shared payloads,
buffers at odd host addresses) through every entry-point form it has: the host form, the list form over three parts that
are laid out in three modes of their own and over three plain slices (which share the whole batch's buffers, so that the
upload sends a span from the middle of each and re-bases the offsets), the resident batch (called twice: the first call
builds the cursor index) or the `_dev` form. Expected: the oracle's grid and aggregates of the canonical layout (one
buffer, payloads back to back in row order; tests/test_layouts_cpu.py shows the oracle's bits do not move with the
layout), numpy on that grid for the selections, and - bit for bit, SUM as float64 bytes included - the same HIP call on
the canonical layout. Bit equality and exact integers only: there is no tolerance in this file.
"""

import ctypes

import numpy as np
import pytest

import binned_cases as bc
import comoments_cases as cc
import episodes_cases as ec
import integral_cases as ic
import layouts
import oracle_lib as ora
import resident_orders as ro
import sample_cases as sc
import trend_cases as tc
import modelardb_rs_amd as mdb
from modelardb_rs_amd import MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM

pytestmark = pytest.mark.gpu

ALL = MDB_AGG_COUNT | MDB_AGG_MIN | MDB_AGG_MAX | MDB_AGG_SUM
SEED = 0
F32_MAX = np.float32(np.finfo(np.float32).max)
QUANTILES = (0.0, 0.5, 0.999, 1.0)
DECODER_SWITCHES = ("MDB_GRID_MV_HOST_MIN_VALUES", "MDB_GRID_MV_MIN_VALUES", "MDB_GRID_MV_INDEX")
DECODERS = {
    "default": {},
    # cursors into the MacaqueV streams of host batches left by the call's host threads, every stream
    "host-cursors": {"MDB_GRID_MV_HOST_MIN_VALUES": "1", "MDB_GRID_MV_MIN_VALUES": "8"},
    # no cursor index: the serial and the speculative decoder
    "no-index": {"MDB_GRID_MV_INDEX": "0", "MDB_GRID_MV_MIN_VALUES": "8"},
}


def _set_decoder(monkeypatch, name):
    for switch in DECODER_SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    for switch, value in DECODERS[name].items():
        monkeypatch.setenv(switch, value)
    monkeypatch.delenv("MDB_SEGMENTS_MERGE_LIMIT", raising=False)
    return name


@pytest.fixture(params=list(DECODERS))
def decoder(request, monkeypatch):
    return _set_decoder(monkeypatch, request.param)


@pytest.fixture
def default_decoder(monkeypatch):
    return _set_decoder(monkeypatch, "default")


def _keys(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def _floats_of_keys(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return (keys ^ ((keys >> 31) & 0x7FFFFFFF)).astype(np.int32).view(np.float32)


def _state_bits(state):
    return bytes(ctypes.string_at(ctypes.addressof(state), ctypes.sizeof(state)))


def _count_min_max(state):
    return int(state.count), int(np.float32(state.min).view(np.uint32)), int(np.float32(state.max).view(np.uint32))


def _np_count_min_max(values):
    """COUNT / MIN / MAX of a selection of the oracle's grid, from fresh states (as tests/test_gpu_value_filter.py)."""
    values = np.asarray(values, dtype=np.float32)
    low = np.fmin.reduce(values, initial=F32_MAX) if len(values) else F32_MAX
    high = np.fmax.reduce(values, initial=-F32_MAX) if len(values) else -F32_MAX
    return len(values), int(np.float32(low).view(np.uint32)), int(np.float32(high).view(np.uint32))


def _grid_bits(result):
    """A grid result with its arrays as bytes: (timestamps or None, values[, rows per segment[, metrics]])."""
    return tuple(item if isinstance(item, dict) or item is None else np.ascontiguousarray(item).tobytes()
                 for item in result)


class World:
    """The corpus in the canonical layout, the oracle's results on it, and caches of the relaid batches and of the
    canonical layout's HIP results (computed once per form and decoder setting, then left unchanged)."""

    def __init__(self):
        self.batch, self.timestamps, self.values = layouts.corpus()
        layouts.corpus_conditions(self.batch)
        self.ts, self.val, self.rows, self.metrics = ora.grid_batch(self.batch)
        self.keys = _keys(self.val)
        self.segment = np.repeat(np.arange(len(self.batch)), self.rows.astype(np.int64))
        self.groups = (np.arange(len(self.batch)) % 3).astype(np.uint32)
        self.cuts = layouts.part_cuts(len(self.batch))
        # Time ranges that begin and end inside a piece of a long stream: inside the first long stream; from inside
        # the first to inside the second; from the model segments in front to the middle of the third.
        lengths = layouts.macaque_v_lengths(self.batch)
        rows = np.flatnonzero(self.batch.model_type_id == mdb.MDB_MACAQUE_V_ID)[lengths >= 4097]
        assert len(rows) >= 3
        start, end = self.batch.start_time[rows].tolist(), self.batch.end_time[rows].tolist()
        self.long_rows = rows
        self.ranges = [(start[0] + 7_050, start[0] + 100 * (64 * 40 + 17) + 3),
                       (start[0] + 100_001, end[1] - 33_301),
                       (int(self.ts[len(self.ts) // 7]), start[2] + (end[2] - start[2]) // 2)]
        for lo, hi in self.ranges:
            assert 64 < int(self.inside(lo, hi).sum()) < len(self.ts)
        self._relaid, self._parts, self._canonical = {}, {}, {}

    def inside(self, t_lo, t_hi):
        return (self.ts >= t_lo) & (self.ts <= t_hi)

    def rows_of(self, keep):
        return np.bincount(self.segment[keep], minlength=len(self.batch)).astype(np.uint32)

    def relaid(self, mode):
        if mode not in self._relaid:
            self._relaid[mode] = layouts.relayout(self.batch, mode, SEED)
        return self._relaid[mode]

    def parts(self, mode):
        """Three parts of the relaid batch, each laid out again in a mode of its own (1 or 2, 3 and about 10 buffers)."""
        if mode not in self._parts:
            self._parts[mode] = layouts.three_parts(self.relaid(mode), mode, SEED)
            counts = sorted(len(part.values.buffers) for part in self._parts[mode])
            assert counts[0] <= 2 and counts[1] == 3 and counts[2] >= 6, (mode, counts)
        return self._parts[mode]

    def other(self, mode):
        """The batch in the layout after `mode`."""
        return self.relaid(layouts.MODES[(layouts.MODES.index(mode) + 1) % len(layouts.MODES)])

    def canonical(self, key, run):
        """run(whole batch, its three parts, another copy) on the canonical layout, once per key."""
        if key not in self._canonical:
            self._canonical[key] = run(self.batch, layouts.cut(self.batch), self.batch)
        return self._canonical[key]

    def select(self, flt):
        """The points of the oracle's grid inside the filter's time range whose value passes (numpy, totalOrder keys)."""
        lo_bits, hi_bits = mdb.value_filter_bits(flt)
        lo = -(1 << 31) if flt.flags & mdb.MDB_VALUE_NO_LO else \
            int(_keys(np.uint32(lo_bits).view(np.float32))) + (1 if flt.flags & mdb.MDB_VALUE_LO_OPEN else 0)
        hi = (1 << 31) - 1 if flt.flags & mdb.MDB_VALUE_NO_HI else \
            int(_keys(np.uint32(hi_bits).view(np.float32))) - (1 if flt.flags & mdb.MDB_VALUE_HI_OPEN else 0)
        return self.inside(flt.t_lo, flt.t_hi) & (self.keys >= lo) & (self.keys <= hi)

    def filters(self):
        """A band that cuts Swing segments (the synthetic series climb and fall between 100 and 200), one that passes
        nothing, bounds with a time range that begins and ends inside long streams."""
        band = mdb.value_filter(lo=130.0, hi=160.0, hi_open=True)
        keep = self.select(band)
        swing = self.batch.model_type_id == mdb.MDB_SWING_ID
        partly = (self.rows_of(keep) > 0) & (self.rows_of(keep) < self.rows) & swing
        assert int(partly.sum()) >= 8
        nothing = mdb.value_filter(lo=1e35, hi=1e36)  # (above the residual tails, below FLT_MAX and the infinities)
        assert not self.select(nothing).any()
        t_lo, t_hi = self.ranges[1]
        bounded = mdb.value_filter(lo=-500.0, hi=500.0, lo_open=True, t_lo=t_lo, t_hi=t_hi)
        assert 0 < int(self.select(bounded).sum()) < int(self.inside(t_lo, t_hi).sum())
        return {"band": band, "nothing": nothing, "bounded": bounded}


@pytest.fixture(scope="module")
def world():
    return World()


def _assert_same(got, canonical, what):
    assert got.keys() == canonical.keys()
    for name in got:
        assert got[name] == canonical[name], (what, name, "differs from the canonical layout's")


# ---- grid -----------------------------------------------------------------------------------------------------------

def _run_grid(hip, world):
    def run(whole, parts, _):
        out = {"count": hip.grid_count(whole), "batch": hip.grid_batch(whole),
               "owned": hip.grid_batch_owned(whole, values_only=True),
               "submit": hip.grid_submit(parts).wait()[:4], "submit cut": hip.grid_submit(layouts.cut(whole)).wait()[:4]}
        for k, (lo, hi) in enumerate(world.ranges):
            out[f"range {k}"] = hip.grid_batch_range(whole, lo, hi)
            out[f"owned range {k}"] = hip.grid_batch_owned(whole, time_range=(lo, hi))
        lo, hi = world.ranges[1]
        out["submit range"] = hip.grid_submit(parts, time_range=(lo, hi)).wait()[:4]
        resident = hip.upload_segments(whole)
        try:
            for call in (1, 2):  # (the first call builds the cursor index)
                out[f"resident {call}"] = hip.grid_resident(resident)
                for k, time_range in enumerate(world.ranges):
                    out[f"resident {call} range {k}"] = hip.grid_resident(resident, time_range)
        finally:
            resident.free()
        return {name: result if name == "count" else _grid_bits(result) for name, result in out.items()}
    return run


@pytest.mark.parametrize("mode", layouts.MODES)
def test_grid(hip, world, decoder, mode):
    run = _run_grid(hip, world)
    got = run(world.relaid(mode), world.parts(mode), None)
    # the oracle's timestamps and value bits, its rows per segment and its counters
    whole = _grid_bits((world.ts, world.val, world.rows, world.metrics))
    assert got["count"] == len(world.ts)
    assert got["batch"] == whole and got["submit"] == whole and got["submit cut"] == whole, (mode, decoder)
    assert got["owned"][:3] == (None,) + whole[1:3], (mode, decoder)
    assert got["resident 1"] == whole[:2] and got["resident 2"] == whole[:2], (mode, decoder)
    for k, (lo, hi) in enumerate(world.ranges):
        keep = world.inside(lo, hi)
        expected = _grid_bits((world.ts[keep], world.val[keep], world.rows_of(keep)))
        assert got[f"range {k}"][:3] == expected and got[f"owned range {k}"][:3] == expected, (mode, decoder, k)
        assert got[f"resident 1 range {k}"] == expected[:2] and got[f"resident 2 range {k}"] == expected[:2], (mode, decoder, k)
        if k == 1:
            assert got["submit range"][:3] == expected, (mode, decoder)
    # everything, the counters of the ranged and submitted forms included, as the canonical layout gives it
    _assert_same(got, world.canonical(("grid", decoder), run), (mode, decoder))


# ---- aggregates -----------------------------------------------------------------------------------------------------

def _run_agg(hip, world):
    def run(whole, parts, _):
        cut = layouts.cut(whole)
        out = {"batch": hip.agg_batch(whole, ALL), "list": hip.agg_batch_list(parts, ALL),
               "list cut": hip.agg_batch_list(cut, ALL)}
        for k, (lo, hi) in enumerate(world.ranges):
            out[f"range {k}"] = hip.agg_batch_range(whole, lo, hi, ALL)
            out[f"range list {k}"] = hip.agg_batch_range_list(parts, lo, hi, ALL)
            out[f"range list cut {k}"] = hip.agg_batch_range_list(cut, lo, hi, ALL)
        resident = hip.upload_segments(whole)
        try:
            for call in ("dev", "dev with index"):
                out[call] = hip.agg_batch_dev(resident, ALL)
                for k, (lo, hi) in enumerate(world.ranges):
                    out[f"{call} range {k}"] = hip.agg_batch_range_dev(resident, lo, hi, ALL)
                hip.grid_resident(resident)  # (builds the cursor index the second round finds)
        finally:
            resident.free()
        return {name: (_state_bits(state), _count_min_max(state)) for name, state in out.items()}
    return run


@pytest.mark.parametrize("mode", layouts.MODES)
def test_aggregates(hip, world, decoder, mode):
    run = _run_agg(hip, world)
    got = run(world.relaid(mode), world.parts(mode), None)
    whole = _count_min_max(ora.agg_batch(world.batch, ALL))
    ranged = [_count_min_max(ora.agg_batch_range(world.batch, lo, hi, ALL)) for lo, hi in world.ranges]
    for name, (_, count_min_max) in got.items():
        expected = ranged[int(name[-1])] if "range" in name else whole
        assert count_min_max == expected, (mode, decoder, name, "COUNT / MIN / MAX differ from the oracle's")
    # SUM as float64 bytes: the canonical layout's from the same form and setting
    _assert_same(got, world.canonical(("agg", decoder), run), (mode, decoder))


# ---- value filters --------------------------------------------------------------------------------------------------

def _run_filters(hip, world):
    def run(whole, parts, _):
        out = {}
        resident = hip.upload_segments(whole)
        try:
            for name, flt in world.filters().items():
                out[f"grid {name}"] = _grid_bits(hip.grid_filter(whole, flt))
                for call in (1, 2):
                    out[f"grid resident {call} {name}"] = _grid_bits(hip.grid_filter_resident(resident, flt))
                states = {"agg": hip.agg_filter(whole, flt, ALL), "agg list": hip.agg_filter_list(parts, flt, ALL),
                          "agg list cut": hip.agg_filter_list(layouts.cut(whole), flt, ALL),
                          "agg dev": hip.agg_filter_dev(resident, flt, ALL)}
                for form, state in states.items():
                    out[f"{form} {name}"] = (_state_bits(state), _count_min_max(state))
        finally:
            resident.free()
        return out
    return run


@pytest.mark.parametrize("mode", layouts.MODES)
def test_value_filters(hip, world, default_decoder, mode):
    run = _run_filters(hip, world)
    got = run(world.relaid(mode), world.parts(mode), None)
    for name, flt in world.filters().items():
        keep = world.select(flt)
        rows = _grid_bits((world.ts[keep], world.val[keep], world.rows_of(keep)))
        for form in ("grid", "grid resident 1", "grid resident 2"):
            assert got[f"{form} {name}"][:3] == rows, (mode, form, name)
        for form in ("agg", "agg list", "agg list cut", "agg dev"):
            assert got[f"{form} {name}"][1] == _np_count_min_max(world.val[keep]), (mode, form, name)
    _assert_same(got, world.canonical("filters", run), mode)


# ---- row masks ------------------------------------------------------------------------------------------------------

def _run_masks(hip, world):
    def run(whole, _, other):
        out = {}
        resident = hip.upload_segments(whole)
        try:
            for name, flt in world.filters().items():
                n_rows = int(world.inside(flt.t_lo, flt.t_hi).sum())
                words = mdb.mask_words(n_rows)
                mask = hip.upload_array(np.full((words + 1) * 8, 0xFF, dtype=np.uint8))  # (one guard word behind)
                try:
                    out[f"mask {name}"] = hip.mask_filter_dev(resident, flt, mask, words)
                    out[f"mask bits {name}"] = hip.download_mask(mask, n_rows, with_padding=True).tobytes()
                    out[f"guard {name}"] = hip.download_array(mask, 8, np.uint8, offset_elements=words * 8).tobytes()
                    n_set = out[f"mask {name}"][1]
                    out[f"grid mask {name}"] = _grid_bits(hip.grid_mask_resident(resident, flt.t_lo, flt.t_hi, mask, n_rows, n_set))
                    state = hip.agg_mask_dev(resident, flt.t_lo, flt.t_hi, mask, n_rows, ALL)
                    out[f"agg mask {name}"] = (_state_bits(state), _count_min_max(state))
                finally:
                    hip.dev_free(mask)
                # predicate and target: the same batch in DIFFERENT layouts
                state = hip.agg_where([whole], [flt], other, ALL)
                out[f"agg where {name}"] = (_state_bits(state), _count_min_max(state))
                out[f"grid where {name}"] = _grid_bits(hip.grid_where([whole], [flt], other))
        finally:
            resident.free()
        return out
    return run


@pytest.mark.parametrize("mode", layouts.MODES)
def test_row_masks(hip, world, default_decoder, mode):
    run = _run_masks(hip, world)
    got = run(world.relaid(mode), None, world.other(mode))
    for name, flt in world.filters().items():
        inside = world.inside(flt.t_lo, flt.t_hi)
        keep = world.select(flt)
        n_rows, n_set = int(inside.sum()), int(keep.sum())
        assert got[f"mask {name}"] == (n_rows, n_set), (mode, name)
        bits = np.zeros(mdb.mask_words(n_rows) * 64, dtype=bool)  # (the padding bits are zero)
        bits[:n_rows] = keep[inside]
        assert got[f"mask bits {name}"] == bits.tobytes(), (mode, name)
        assert got[f"guard {name}"] == b"\xff" * 8, (mode, name)
        rows = _grid_bits((world.ts[keep], world.val[keep], world.rows_of(keep)))
        assert got[f"grid mask {name}"][:3] == rows and got[f"grid where {name}"][:3] == rows, (mode, name)
        for form in ("agg mask", "agg where"):
            assert got[f"{form} {name}"][1] == _np_count_min_max(world.val[keep]), (mode, form, name)
    _assert_same(got, world.canonical("masks", run), mode)


# ---- aggregates per bucket ------------------------------------------------------------------------------------------

def _bucket_sets(world):
    """(origin, width, n_buckets, t_lo, t_hi): a width that cuts the long streams a dozen times each, over them alone;
    wide buckets from the first point on, under a time range."""
    first = int(world.batch.start_time[world.long_rows[0]]) - 5_000
    last = int(world.batch.end_time[world.long_rows[-1]])
    fine = (first, 33_333, (last - first) // 33_333 + 2, None, None)
    wide = (int(world.ts[0]) - 7, 777_777, 40, world.ranges[2][0], world.ranges[2][1])
    return {"fine": fine, "wide": wide}


def _run_buckets(hip, world):
    def run(whole, parts, _):
        out = {}
        groups = world.groups
        part_groups = [groups[world.cuts[k]:world.cuts[k + 1]] for k in range(3)]
        flt = world.filters()["band"]
        resident = hip.upload_segments(whole)
        try:
            for name, (origin, width, n_buckets, t_lo, t_hi) in _bucket_sets(world).items():
                args = dict(t_lo=t_lo, t_hi=t_hi, n_groups=3)
                out[f"host {name}"] = hip.agg_buckets(whole, origin, width, n_buckets, groups, **args)
                out[f"list {name}"] = hip.agg_buckets_list(parts, origin, width, n_buckets, part_groups, **args)
                out[f"list cut {name}"] = hip.agg_buckets_list(layouts.cut(whole), origin, width, n_buckets, part_groups, **args)
                out[f"dev {name}"] = hip.agg_buckets_dev(resident, origin, width, n_buckets, groups, **args)
                out[f"filter host {name}"] = hip.agg_buckets_filter(whole, flt, origin, width, n_buckets, groups, **args)
                out[f"filter list {name}"] = hip.agg_buckets_filter_list(parts, flt, origin, width, n_buckets, part_groups, **args)
                out[f"filter list cut {name}"] = hip.agg_buckets_filter_list(layouts.cut(whole), flt, origin, width, n_buckets,
                                                                             part_groups, **args)
                out[f"filter dev {name}"] = hip.agg_buckets_filter_dev(resident, flt, origin, width, n_buckets, groups, **args)
        finally:
            resident.free()
        return {name: (cells.tobytes(), cells["count"].tobytes()) for name, cells in out.items()}
    return run


@pytest.mark.parametrize("mode", layouts.MODES)
def test_bucket_aggregates(hip, world, default_decoder, mode):
    run = _run_buckets(hip, world)
    got = run(world.relaid(mode), world.parts(mode), None)
    point_groups = world.groups.astype(np.int64)[world.segment]
    passing = world.select(world.filters()["band"])
    for name, (origin, width, n_buckets, t_lo, t_hi) in _bucket_sets(world).items():
        buckets = (world.ts - origin) // width  # (date_bin's floor; every timestamp is far from the ends of int64)
        keep = (buckets >= 0) & (buckets < n_buckets)
        if t_lo is not None:
            keep &= world.inside(t_lo, t_hi)
        for form, selected in (("", keep), ("filter ", keep & passing)):
            counts = np.bincount(point_groups[selected] * n_buckets + buckets[selected], minlength=3 * n_buckets)
            assert counts.max() > 8 and (counts > 0).sum() >= 16  # (the expectation itself: many cells hold points)
            for where in ("host", "list", "list cut", "dev"):
                assert got[f"{form}{where} {name}"][1] == counts.astype(np.int64).tobytes(), (mode, form, where, name)
    # all cells' bytes: COUNT, MIN, MAX and SUM as the canonical layout gives them
    _assert_same(got, world.canonical("buckets", run), mode)


# ---- histograms and quantiles ---------------------------------------------------------------------------------------

def _edge_lists(world):
    """Seven edges ON rebuilt values and on their f32 neighbours; 4 095 edges even in key space between the grid's
    smallest and largest key (the lists of tests/test_gpu_hist.py)."""
    ordered = np.sort(world.keys)
    on_values = _floats_of_keys(ordered[[len(ordered) // 5, len(ordered) // 2, (4 * len(ordered)) // 5]])
    with np.errstate(over="ignore", invalid="ignore"):
        around = np.concatenate([np.nextafter(on_values, np.float32(-np.inf)), on_values,
                                 np.nextafter(on_values, np.float32(np.inf))])
    seven = _floats_of_keys(np.unique(_keys(around))[:7])
    lo, hi = int(ordered[0]), int(ordered[-1])
    picked = np.unique(np.linspace(lo, hi, 4095 + 2)[1:-1].astype(np.int64))
    many = _floats_of_keys(picked[(picked > lo) & (picked <= hi)])
    assert len(seven) == 7 and len(many) == 4095
    return {"7": seven, "4095": many}


@pytest.mark.parametrize("mode", layouts.MODES)
def test_histograms_and_quantiles(hip, world, default_decoder, mode):
    # (No comparison with the canonical layout's HIP result here, on purpose: counts and order statistics are exact
    # integers and bit patterns, so equality with numpy on the oracle's grid already implies it.)
    whole, parts = world.relaid(mode), world.parts(mode)
    groups = world.groups
    part_groups = [groups[world.cuts[k]:world.cuts[k + 1]] for k in range(3)]
    point_groups = groups.astype(np.int64)[world.segment]
    resident = hip.upload_segments(whole)
    try:
        for t_lo, t_hi in [(None, None), world.ranges[1], world.ranges[2]]:
            keep = np.ones(len(world.ts), dtype=bool) if t_lo is None else world.inside(t_lo, t_hi)
            for name, edges in _edge_lists(world).items():
                cells = np.searchsorted(_keys(edges), world.keys[keep], side="right")
                n_cells = len(edges) + 1
                expected = np.bincount(point_groups[keep] * n_cells + cells, minlength=3 * n_cells).astype(np.uint64)
                expected = expected.reshape(3, n_cells)
                case = (mode, name, t_lo, t_hi)
                assert np.array_equal(hip.hist(whole, edges, groups, t_lo, t_hi, n_groups=3), expected), case
                assert np.array_equal(hip.hist_list(parts, edges, part_groups, t_lo, t_hi, n_groups=3), expected), case
                assert np.array_equal(hip.hist_list(layouts.cut(whole), edges, part_groups, t_lo, t_hi, n_groups=3), expected), case
                for _ in range(2):
                    assert np.array_equal(hip.hist_dev(resident, edges, groups, t_lo, t_hi, n_groups=3), expected), case
            ordered = np.sort(world.keys[keep])
            n = len(ordered)
            positions = [(int(np.floor(np.float64(q) * np.float64(n - 1))), int(np.ceil(np.float64(q) * np.float64(n - 1))))
                         for q in QUANTILES]
            expected_lo = _floats_of_keys(ordered[[p[0] for p in positions]]).tobytes()
            expected_hi = _floats_of_keys(ordered[[p[1] for p in positions]]).tobytes()
            for lo, hi, n_points in (hip.quantile(whole, QUANTILES, t_lo, t_hi),
                                     hip.quantile_dev(resident, QUANTILES, t_lo, t_hi)):
                assert n_points == n and lo.tobytes() == expected_lo and hi.tobytes() == expected_hi, (mode, t_lo, t_hi)
    finally:
        resident.free()


# ---- the later operators: two fields, trends, episodes, integrals, samples ------------------------------------------
# Requests: the two runs of buckets (or instants) of tests/resident_orders.py's corpus, in front of and behind the
# corpus's gaps of 2^40. Per operator the canonical layout's host form is held to the operator's reference and its
# test file's tolerance once; every form - on the canonical layout and on a relaid batch - then gives the bytes of
# that one answer. The pair operators get x and y in DIFFERENT layouts, and lists cut at different rows: three parts of x
# against two of y.

class Later:
    """What the later operators are asked about the corpus, and their references (computed once)."""

    def __init__(self, world):
        self.world = world
        self.corpus = ro.corpus_a()
        assert self.corpus.batch is world.batch                          # (layouts.corpus(), cached)
        self.partner = self.corpus.partner.batch                         # the same series times 1.5: other segments
        self.partner_groups = (np.arange(len(self.partner)) % 3).astype(np.uint32)
        self.run_groups = ((np.arange(len(world.batch)) // ro.GROUP_RUN) % 3).astype(np.uint32)
        self.edges = self.corpus.partner.edges
        self.field, self.partner_field = cc.Field([world.batch]), cc.Field([self.partner])
        self._relaid, self._parts, self._checked = {}, {}, {}

    def partner_relaid(self, mode):
        if mode not in self._relaid:
            self._relaid[mode] = layouts.relayout(self.partner, mode, SEED + 11)
        return self._relaid[mode]

    def partner_parts(self, mode):
        if mode not in self._parts:
            self._parts[mode] = layouts.three_parts(self.partner_relaid(mode), mode, SEED + 11)
        return self._parts[mode]

    halves = staticmethod(layouts.halves)
    groups_of_parts = staticmethod(layouts.groups_of_parts)

    def canonical(self, key, run, check):
        """run(...) on the canonical layout, once per key: its host form held to the reference by check(result), its
        list and dev forms to the bytes of the host form (the contract: the three forms agree bit for bit)."""
        if key not in self._checked:
            result = run(None)
            check(result)
            _assert_forms(result, result, "canonical")
            self._checked[key] = result
        return self._checked[key]


@pytest.fixture(scope="module")
def later(world):
    return Later(world)


def _bytes_of(results):
    return {name: [np.ascontiguousarray(item).tobytes() if isinstance(item, np.ndarray) else item for item in
                   (result if isinstance(result, (list, tuple)) else [result])] for name, result in results.items()}


def _assert_forms(got, canonical, mode):
    """Every form of `got` ("host", "list", "dev", with the request's number behind) has the bytes of the canonical
    layout's HOST form of the same request: the one answer that is tied to the reference."""
    got, canonical = _bytes_of(got), _bytes_of(canonical)
    assert got.keys() == canonical.keys() and len(got) % 3 == 0
    for name in got:
        anchored = "host" + name[len(name.split()[0]):]
        assert name.split()[0] in ("host", "list", "dev") and anchored in canonical
        assert got[name] == canonical[anchored], (mode, name, "differs from the canonical layout's host form")


def _next_mode(mode):
    return layouts.MODES[(layouts.MODES.index(mode) + 1) % len(layouts.MODES)]


def _run_pair(hip, later, operator):
    """comoments: x = the corpus, y = its partner; binned: x = the partner, y = the corpus. The host, list and dev forms
    per span; mode None: both in the canonical layout."""
    world = later.world
    extra = () if operator == "comoments" else (later.edges,)
    host, listed, dev = [getattr(hip, f"{operator}_buckets{form}") for form in ("", "_list", "_dev")]

    def run(mode):
        if operator == "comoments":
            x = world.batch if mode is None else world.relaid(mode)
            y = later.partner if mode is None else later.partner_relaid(_next_mode(mode))
            xs = layouts.cut(x) if mode is None else world.parts(mode)
            groups = world.groups
        else:
            x = later.partner if mode is None else later.partner_relaid(mode)
            y = world.batch if mode is None else world.relaid(_next_mode(mode))
            xs = layouts.cut(x) if mode is None else later.partner_parts(mode)
            groups = later.partner_groups
        ys = later.halves(y)
        out = {}
        dev_x, dev_y = hip.upload_segments(x), hip.upload_segments(y)
        try:
            for k, span in enumerate(later.corpus.spans):
                out[f"host {k}"] = host(x, y, *extra, *span, groups=groups, n_groups=3)
                out[f"list {k}"] = listed(xs, ys, *extra, *span, groups=later.groups_of_parts(groups), n_groups=3)
                out[f"dev {k}"] = dev(dev_x, dev_y, *extra, *span, groups=groups, n_groups=3)
        finally:
            dev_x.free()
            dev_y.free()
        return out
    return run


@pytest.mark.parametrize("mode", layouts.MODES)
def test_comoments(hip, world, later, default_decoder, mode):
    run = _run_pair(hip, later, "comoments")

    def check(canonical):
        for k, span in enumerate(later.corpus.spans):
            expected = cc.oracle(later.field, later.partner_field, world.groups, 3, *span)
            assert int((expected["count"] > 0).sum()) > 100
            cc.assert_cells(canonical[f"host {k}"], expected, f"comoments, span {k}")

    _assert_forms(run(mode), later.canonical("comoments", run, check), mode)


@pytest.mark.parametrize("mode", layouts.MODES)
def test_binned(hip, world, later, default_decoder, mode):
    run = _run_pair(hip, later, "binned")

    def check(canonical):
        for k, span in enumerate(later.corpus.spans):
            expected = bc.oracle(later.partner_field, later.field, later.edges, later.partner_groups, 3, *span)
            assert int((expected["count"] > 0).sum()) > 100
            bc.assert_cells(canonical[f"host {k}"], expected, f"binned, span {k}")

    _assert_forms(run(mode), later.canonical("binned", run, check), mode)


def _run_single(hip, later, calls, spans, groups, **arguments):
    """The host, list and dev forms of an operator on one batch, per span; mode None: the canonical layout."""
    world = later.world
    host, listed, dev = calls

    def run(mode):
        whole = world.batch if mode is None else world.relaid(mode)
        parts = layouts.cut(whole) if mode is None else world.parts(mode)
        out = {}
        resident = hip.upload_segments(whole)
        try:
            for k, span in enumerate(spans):
                out[f"host {k}"] = host(whole, *span, groups=groups, n_groups=3, **arguments)
                out[f"list {k}"] = listed(parts, *span, groups=later.groups_of_parts(groups), n_groups=3, **arguments)
                out[f"dev {k}"] = dev(resident, *span, groups=groups, n_groups=3, **arguments)
        finally:
            resident.free()
        return out
    return run


@pytest.mark.parametrize("mode", layouts.MODES)
def test_trend(hip, world, later, default_decoder, mode):
    run = _run_single(hip, later, (hip.trend_buckets, hip.trend_buckets_list, hip.trend_buckets_dev), later.corpus.spans,
                      world.groups)

    def check(canonical):
        special = 0
        for k, span in enumerate(later.corpus.spans):
            expected = tc.oracle(later.field, world.groups, 3, *span)
            cc.assert_cells(canonical[f"host {k}"], expected, f"trend, span {k}")
            special += tc.assert_x_side(canonical[f"host {k}"], expected, f"trend, span {k}")
        assert special > 0

    _assert_forms(run(mode), later.canonical("trend", run, check), mode)


@pytest.mark.parametrize("mode", layouts.MODES)
def test_integral(hip, world, later, default_decoder, mode):
    arguments = dict(method=mdb.MDB_INTEGRAL_LINEAR, max_gap=ro.LINK_GAP)
    run = _run_single(hip, later, (hip.integral_buckets, hip.integral_buckets_list, hip.integral_buckets_dev),
                      later.corpus.spans, later.run_groups, **arguments)

    def check(canonical):
        special = 0
        for k, span in enumerate(later.corpus.spans):
            expected = ic.oracle(later.field, later.run_groups, 3, *span, ic.LINEAR, ro.LINK_GAP)
            special += ic.assert_cells(canonical[f"host {k}"], expected, f"integral, span {k}")[1]
        assert special > 0

    _assert_forms(run(mode), later.canonical("integral", run, check), mode)


@pytest.mark.parametrize("mode", layouts.MODES)
def test_sample(hip, world, later, default_decoder, mode):
    arguments = dict(method=mdb.MDB_SAMPLE_LINEAR, max_gap=ro.LINK_GAP)
    run = _run_single(hip, later, (hip.sample_at, hip.sample_at_list, hip.sample_at_dev), later.corpus.sample_spans,
                      later.run_groups, **arguments)

    def check(canonical):
        special = 0
        for k, span in enumerate(later.corpus.sample_spans):
            expected = sc.oracle(later.field, later.run_groups, 3, *span, sc.LINEAR, ro.LINK_GAP)
            special += sc.assert_cells(canonical[f"host {k}"], expected, f"sample, span {k}")[1]
        assert special > 0

    _assert_forms(run(mode), later.canonical("sample", run, check), mode)


@pytest.mark.parametrize("mode", layouts.MODES)
def test_episodes(hip, world, later, default_decoder, mode):
    band = world.filters()["band"]
    arguments = dict(n_groups=3, max_gap=ro.EPISODE_GAP)

    def run(mode):
        whole = world.batch if mode is None else world.relaid(mode)
        parts = layouts.cut(whole) if mode is None else world.parts(mode)
        resident = hip.upload_segments(whole)
        try:
            return {"host": hip.episodes(whole, band, later.run_groups, **arguments),
                    "list": hip.episodes_list(parts, band, later.groups_of_parts(later.run_groups), **arguments),
                    "dev": hip.episodes_dev(resident, band, later.run_groups, **arguments)}
        finally:
            resident.free()

    def check(canonical):
        expected, magnitudes, n_rows, n_passing, _ = ec.reference(ec.Table(world.batch), band, groups=later.run_groups,
                                                                  max_gap=ro.EPISODE_GAP)
        episodes, rows, passing = canonical["host"]
        assert (rows, passing) == (n_rows, n_passing) and len(expected) > 100
        ec.assert_episodes(episodes, expected, magnitudes)

    _assert_forms(run(mode), later.canonical("episodes", run, check), mode)


# ---- upload and download ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("merge_limit", [None, "4096"], ids=["merged", "apart"])
@pytest.mark.parametrize("mode", layouts.MODES)
def test_download(hip, world, default_decoder, monkeypatch, mode, merge_limit):
    if merge_limit is not None:
        monkeypatch.setenv("MDB_SEGMENTS_MERGE_LIMIT", merge_limit)  # (the buffers come back one by one)
    resident = hip.upload_segments(world.relaid(mode))
    try:
        hip.validate_segments_dev(resident)
        back = resident.download()
        assert back.identical(world.batch), mode
        for name in layouts.COLUMNS:  # (one buffer per column, or the buffers one by one as they were sent)
            expected = 1 if merge_limit is None else len(getattr(world.relaid(mode), name).buffers)
            assert len(getattr(back, name).buffers) == expected, (mode, name)
    finally:
        resident.free()
