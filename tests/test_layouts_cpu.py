"""The re-layout helper of the layout-invariance tier (tests/layouts.py), held to what it promises where no GPU is at
hand: every mode keeps every payload byte, gives arrow a valid BinaryViewArray, survives the round trip through arrow,
and leaves the oracle's grid and aggregates bit for bit as they are; the corpus holds what tests/test_gpu_layouts.py
relies on."""

import ctypes

import numpy as np
import pytest

import layouts
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM

ALL = MDB_AGG_COUNT | MDB_AGG_MIN | MDB_AGG_MAX | MDB_AGG_SUM
SEEDS = (0, 1)


def _state_bits(state):
    return bytes(ctypes.string_at(ctypes.addressof(state), ctypes.sizeof(state)))


@pytest.fixture(scope="module")
def canonical():
    batch, timestamps, values = layouts.corpus()
    grid = ora.grid_batch(batch)
    ordered = np.sort(grid[0])
    ranges = [(int(ordered[len(ordered) // 7]), int(ordered[len(ordered) // 3])),
              (int(ordered[-4000]), int(ordered[-1]))]
    return {"batch": batch, "timestamps": timestamps, "values": values, "grid": grid,
            "agg": _state_bits(ora.agg_batch(batch, ALL)),
            "ranges": [(lo, hi, _state_bits(ora.agg_batch_range(batch, lo, hi, ALL))) for lo, hi in ranges]}


def test_corpus_conditions(canonical):
    batch = canonical["batch"]
    layouts.corpus_conditions(batch, SEEDS)
    # lossless parts come back as they went in; the whole is one ascending series
    timestamps, values = canonical["grid"][0], canonical["grid"][1]
    assert np.array_equal(timestamps, canonical["timestamps"]) and np.all(np.diff(timestamps) >= 0)
    assert len(values) == len(canonical["values"])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mode", layouts.MODES)
def test_relayout_keeps_every_byte_and_the_oracles_bits(canonical, mode, seed):
    batch = canonical["batch"]
    relaid = layouts.relayout(batch, mode, seed)
    assert batch.identical(relaid) and relaid.identical(batch)
    for name in layouts.COLUMNS:
        column = getattr(relaid, name)
        column.to_arrow().validate(full=True)
        lengths = column.lengths()
        words = column.views.view(np.int32).reshape(-1, 4)
        # 12 bytes or fewer inline, padded with zeros; everything else inside its buffer
        inline = lengths <= 12
        for row in np.flatnonzero(inline):
            assert not column.views[row, 4 + lengths[row]:].any()
        sizes = np.array([len(b) for b in column.buffers], dtype=np.int64)
        assert np.all(words[~inline, 2] >= 0) and np.all(words[~inline, 2] < len(sizes))
        assert np.all(words[~inline, 3] >= 0)
        assert np.all(words[~inline, 3].astype(np.int64) + lengths[~inline] <= sizes[words[~inline, 2]])
        if mode == "empty-first":
            assert len(column.buffers[0]) == 0 and not np.any(words[~inline, 2] == 0)
        if mode == "odd-base":
            assert all(b.ctypes.data % 16 != 0 for b in column.buffers if len(b))
        if mode != "blocks":
            # one payload begins at byte 0 and one ends at the last byte of every buffer that holds any
            for b, size in enumerate(sizes):
                here = ~inline & (words[:, 2] == b)
                if size:
                    assert np.any(words[here, 3] == 0) and np.any(words[here, 3] + lengths[here] == size)
        if mode in ("padded-one", "three", "empty-first", "odd-base"):
            # the filler between the payloads is never zero
            covered = [np.zeros(size, dtype=bool) for size in sizes]
            for row in np.flatnonzero(~inline):
                covered[words[row, 2]][words[row, 3]:words[row, 3] + lengths[row]] = True
            for buffer, mask in zip(column.buffers, covered):
                assert np.all(buffer[~mask] == layouts.FILLER)
    if mode == "blocks":
        assert all(8 <= len(getattr(relaid, name).buffers) <= 16 for name in layouts.COLUMNS)
    back = mdb.SegmentBatch.from_arrow(relaid.to_arrow())
    assert back.identical(batch)
    for name in layouts.COLUMNS:
        assert len(getattr(back, name).buffers) == len(getattr(relaid, name).buffers)
    got = ora.grid_batch(relaid)
    expected = canonical["grid"]
    assert np.array_equal(got[0], expected[0])
    assert np.array_equal(got[1].view(np.uint32), expected[1].view(np.uint32))
    assert np.array_equal(got[2], expected[2]) and got[3] == expected[3]
    assert _state_bits(ora.agg_batch(relaid, ALL)) == canonical["agg"]
    for lo, hi, bits in canonical["ranges"]:
        assert _state_bits(ora.agg_batch_range(relaid, lo, hi, ALL)) == bits


def test_shared_rows_point_at_one_copy(canonical):
    batch = canonical["batch"]
    relaid = layouts.relayout(batch, "shared", 0)
    for name in layouts.COLUMNS:
        items = getattr(batch, name).to_bytes_list()
        words = getattr(relaid, name).views.view(np.int32).reshape(-1, 4)
        where = {}
        for row, item in enumerate(items):
            if len(item) > 12:
                assert where.setdefault(item, (words[row, 2], words[row, 3])) == (words[row, 2], words[row, 3])


def test_three_parts_are_the_batch_in_other_layouts(canonical):
    batch = canonical["batch"]
    for mode in layouts.MODES:
        parts = layouts.three_parts(layouts.relayout(batch, mode, 0), mode, 0)
        assert len(parts) == 3 and all(len(part) > 0 for part in parts)
        assert mdb.SegmentBatch.concat(parts).identical(batch)
        # 1 (or 2), 3 and about 10 buffers: the joint table of a list form shifts indexes unevenly
        counts = sorted(len(part.values.buffers) for part in parts)
        assert counts[0] <= 2 and counts[1] == 3 and counts[2] >= 6, (mode, counts)
        # plain slices share the buffers: what their views touch begins in the middle of a buffer, past the 16 bytes
        # the upload rounds the start of the travelling span down to
        late = 0
        for part in layouts.cut(layouts.relayout(batch, mode, 0)):
            indexes, offsets = layouts.out_of_line_offsets(part.values)
            late += sum(int(offsets[indexes == b].min()) >= 16 for b in np.unique(indexes))
        assert late >= 2, mode


def test_the_lists_of_two_fields_are_cut_at_different_rows(canonical):
    # What tests/test_gpu_layouts.py hands the operators on two fields: three parts of x (layouts.three_parts, their
    # groups by layouts.groups_of_parts) against two parts of y (layouts.halves), x and y the corpus and its partner
    # of tests/resident_orders.py in either role.
    import resident_orders as ro
    corpus = ro.corpus_a()
    assert corpus.batch is canonical["batch"] or corpus.batch.identical(canonical["batch"])
    fields = (corpus.batch, corpus.partner.batch)
    assert len(fields[0]) != len(fields[1])
    for x, y in (fields, fields[::-1]):
        groups = (np.arange(len(x)) % 3).astype(np.uint32)
        for mode in layouts.MODES[:2]:
            parts = layouts.three_parts(layouts.relayout(x, mode, 11), mode, 11)
            part_groups = layouts.groups_of_parts(groups)
            assert [len(g) for g in part_groups] == [len(part) for part in parts] == [len(part) for part in layouts.cut(x)]
            assert np.array_equal(np.concatenate(part_groups), groups)
            assert mdb.SegmentBatch.concat(parts).identical(x)
        two = layouts.halves(y)
        assert len(two) == 2 and all(len(part) > 0 for part in two) and mdb.SegmentBatch.concat(two).identical(y)
        # y's cut is at none of x's part_cuts, neither by row number nor in time: the row behind it begins inside a
        # part of x, away from that part's first row
        assert len(two[0]) not in layouts.part_cuts(len(x)) and len(two[0]) not in layouts.part_cuts(len(y))
        cut_time = int(two[1].start_time[0])
        x_cut_times = [int(x.start_time[row]) for row in layouts.part_cuts(len(x))[1:-1]]
        assert cut_time not in x_cut_times and int(x.start_time[0]) < cut_time < int(x.start_time[-1])
