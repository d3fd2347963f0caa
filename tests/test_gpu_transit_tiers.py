"""transit_buckets on the tiers the other operators are held to in tests/test_gpu_layouts.py and
tests/test_gpu_shard_soak.py: the corpus of tests/layouts.py in six physical layouts of its BinaryView columns, and one
batch cut at series boundaries into several calls on one context - merged in either order, chained by adding into one
array, and interleaved with other operators on the same resident batches. Everything is byte-equal to one call on the
canonical batch, which is held to the reference (tests/transit_cases.py) once."""

import numpy as np
import pytest

import comoments_cases as cc
import dwell_cases as dc
import layouts
import oracle_lib as ora
import transit_cases as tc
import modelardb_rs_amd as mdb

pytestmark = pytest.mark.gpu

SEED = 11


@pytest.fixture(scope="module", autouse=True)
def _resident_copies():
    yield
    cc.free_tables()


class World:
    """The corpus, a group id per segment, two requests, and the canonical layout's results (computed once, compared
    with the reference once, then left unchanged)."""

    def __init__(self, hip):
        self.batch, _, _ = layouts.corpus()
        layouts.corpus_conditions(self.batch)
        ts, values, rows, _ = ora.grid_batch(self.batch)
        self.groups = (np.arange(len(self.batch)) % 3).astype(np.uint32)
        first, last = int(ts.min()), int(ts.max())
        finite = values[np.isfinite(values)]
        narrow = finite[(finite > 90.0) & (finite < 210.0)]   # (the synthetic series climb and fall between 100 and 200)
        # (one series of the corpus is epoch-scale: the buckets lie where the rows are dense, and rows behind them are dropped)
        dense, quarter = int(np.sort(ts)[(7 * len(ts)) // 10]), int(np.sort(ts)[len(ts) // 4])
        self.requests = {"64 buckets, 16 edges": (dc.edges_through(narrow, 16), first - 777, (dense - first + 777) // 64 + 13, 64, None),
                         "3 000 buckets, 1 edge, a gap rule": (np.array([150.0], dtype=np.float32), quarter, 1_700, 3_000, 150)}
        assert all(3 * request[3] * (len(request[0]) + 1) ** 2 < 100_000 for request in self.requests.values())
        row_groups = self.groups.astype(np.int64)[np.repeat(np.arange(len(self.batch)), rows.astype(np.int64))]
        self.canonical = {}
        for name, (edges, origin, width, n_buckets, max_gap) in self.requests.items():
            got = hip.transit_buckets(self.batch, edges, origin, width, n_buckets, groups=self.groups, max_gap=max_gap, n_groups=3)
            expected = tc.rows_oracle(ts, values, edges, n_buckets, origin, width, row_groups.tolist(), 3, max_gap)
            np.testing.assert_array_equal(got, expected, err_msg=name)
            assert int(got.sum()) > 10_000 and int(got.sum()) > int(np.trace(got, axis1=2, axis2=3).sum())
            self.canonical[name] = got


@pytest.fixture(scope="module")
def world(hip):
    return World(hip)


@pytest.mark.parametrize("mode", layouts.MODES)
def test_layouts(hip, world, mode):
    """The host form on the relaid batch, the dev form on its upload, the list form on three parts each laid out in a
    mode of its own and on the relaid batch cut in three: the canonical layout's bytes."""
    relaid = layouts.relayout(world.batch, mode, SEED)
    parts = layouts.three_parts(relaid, mode, SEED)
    part_groups = layouts.groups_of_parts(world.groups)
    dev = hip.upload_segments(relaid)
    try:
        for name, (edges, origin, width, n_buckets, max_gap) in world.requests.items():
            args = (edges, origin, width, n_buckets)
            common = dict(max_gap=max_gap, n_groups=3)
            forms = {"host": hip.transit_buckets(relaid, *args, groups=world.groups, **common),
                     "dev": hip.transit_buckets_dev(dev, *args, groups=world.groups, **common),
                     "list": hip.transit_buckets_list(parts, *args, groups=part_groups, **common),
                     "list cut": hip.transit_buckets_list(layouts.cut(relaid), *args, groups=part_groups, **common)}
            for form, got in forms.items():
                assert got.tobytes() == world.canonical[name].tobytes(), f"{mode}, {name}, {form}"
    finally:
        dev.free()


@pytest.mark.parametrize("n_calls", [2, 3])
def test_a_batch_cut_at_series_boundaries_into_calls(hip, n_calls):
    """The four series of the main table, each a group or all in one group (where they overlap in time), cut into 2 and
    3 calls: folded with transit_merge in both orders, chained by adding into one array, and each call made on a
    resident shard between dwell_buckets_dev, change_buckets_dev and a grid of the same shard - whose results are
    those of the same calls made alone. Every variant has the bytes of the one call."""
    field = cc.main_table()[1]
    batch = field.batch
    bounds = np.concatenate([[0], np.cumsum([len(part) for part in field.parts])])
    cuts = [0, int(bounds[2]), len(batch)] if n_calls == 2 else [0, int(bounds[1]), int(bounds[3]), len(batch)]
    first, last = int(field.ts.min()), int(field.ts.max())
    edges = dc.edges_through(field.values, 16)
    args = (edges, first - 40, 2_900, (last - first + 40) // 2_900 + 1)
    for groups, n_groups in ((field.groups, 4), (None, 1)):
        whole = hip.transit_buckets(batch, *args, groups=groups, n_groups=n_groups)
        np.testing.assert_array_equal(whole, tc.oracle(field, edges, groups, n_groups, *args[1:]))
        shards = [(batch.slice(a, b), None if groups is None else groups[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        alone = [hip.transit_buckets(shard, *args, groups=g, n_groups=n_groups) for shard, g in shards]
        assert all(part.any() for part in alone)
        for order in (alone, alone[::-1]):
            merged = np.zeros_like(whole)
            for part in order:
                mdb.transit_merge(merged, part)
            assert merged.tobytes() == whole.tobytes()
        chained = np.zeros_like(whole)
        for shard, g in shards:
            assert hip.transit_buckets(shard, *args, groups=g, counts=chained, n_groups=n_groups) is chained
        assert chained.tobytes() == whole.tobytes()
        interleaved = np.zeros_like(whole)
        for (shard, g), part in zip(shards, alone):
            dev = hip.upload_segments(shard)
            try:
                dwell_alone = hip.dwell_buckets_dev(dev, *args, groups=g, n_groups=n_groups)
                change_alone = hip.change_buckets_dev(dev, *args[1:], groups=g, n_groups=n_groups)
                grid_alone = hip.grid_resident(dev)
                hip.transit_buckets_dev(dev, *args, groups=g, counts=interleaved, n_groups=n_groups)
                assert hip.dwell_buckets_dev(dev, *args, groups=g, n_groups=n_groups).tobytes() == dwell_alone.tobytes()
                again = hip.transit_buckets_dev(dev, *args, groups=g, n_groups=n_groups)
                assert hip.change_buckets_dev(dev, *args[1:], groups=g, n_groups=n_groups).tobytes() == change_alone.tobytes()
                grid = hip.grid_resident(dev)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(grid[:2], grid_alone[:2]))
                assert again.tobytes() == part.tobytes() == hip.transit_buckets_dev(dev, *args, groups=g, n_groups=n_groups).tobytes()
                np.testing.assert_array_equal(again.sum(axis=(2, 3), dtype=np.uint64), change_alone["count"])
            finally:
                dev.free()
        assert interleaved.tobytes() == whole.tobytes()
