"""The expected-value builders of the scale tier (tests/scale_cases.py) against ora.grid_batch + numpy at small
parameters, and the tiers' preconditions at FULL parameters from the segments' metadata alone (no grid is built)."""

import numpy as np

import oracle_lib as ora
import scale_cases as sc
import modelardb_rs_amd as mdb
from modelardb_rs_amd.segments import BinaryViewColumn, SegmentBatch


def _same_columns(a, b):
    """Views and buffers byte for byte, not only the items they stand for."""
    assert a.identical(b)
    for name in ("timestamps", "values", "residuals"):
        x, y = getattr(a, name), getattr(b, name)
        assert np.array_equal(x.views, y.views), name
        assert len(x.buffers) == len(y.buffers) and all(np.array_equal(p, q) for p, q in zip(x.buffers, y.buffers)), name


def test_binary_view_column_equals_from_bytes_list():
    rng = np.random.default_rng(1)
    for sizes in ([0, 1, 12, 13, 4, 40, 0, 12, 13], [0, 0, 0], [5], [13], list(rng.integers(0, 30, 500))):
        items = [rng.integers(0, 256, int(size), dtype=np.uint8).tobytes() for size in sizes]
        got = sc.binary_view_column(sizes, np.frombuffer(b"".join(items), dtype=np.uint8))
        expected = BinaryViewColumn.from_bytes_list(items)
        assert np.array_equal(got.views, expected.views) and got.to_bytes_list() == items
        assert len(got.buffers) == len(expected.buffers)
        assert all(np.array_equal(p, q) for p, q in zip(got.buffers, expected.buffers))


def test_regular_lengths_are_what_the_oracle_writes_and_reads():
    lengths = [1, 2, 3, 64, 127, 128, 255, 256, 32767, 32768, 1_000_000, (1 << 23) - 1, 1 << 23]
    counts, data = sc.regular_length_bytes(lengths)
    at = 0
    for n, count in zip(lengths, counts):
        written = ora.compress_residual_timestamps(np.arange(n, dtype=np.int64) * 7) if n <= 1_000_000 else None
        mine = data[at:at + count].tobytes()
        at += count
        if written is not None:
            assert mine == written, n
        if n > 2:
            assert ora.seg_len(0, 7 * (n - 1), mine) == n and ora.are_compressed_timestamps_regular(mine)


def test_the_vectorised_constructor_equals_from_rows():
    rng = np.random.default_rng(2)
    n = 3000
    lengths, deltas = rng.integers(1, 300, n), rng.integers(1, 2000, n)
    lengths[:5] = [1, 2, 3, 127, 128]
    starts = np.cumsum(lengths * deltas + rng.integers(1, 50, n)) - lengths * deltas
    types, first, last, decreasing = sc._simple_values(rng, n)
    rows = []
    for k in range(n):  # the rows of _short_simple_segments (tests/test_gpu_grid.py), written one by one
        length, start, delta = int(lengths[k]), int(starts[k]), int(deltas[k])
        timestamps = b"" if length <= 2 else ora.compress_residual_timestamps(start + np.arange(length, dtype=np.int64) * delta)
        if types[k] == 0 or length == 1:
            rows.append((0, start, start + (length - 1) * delta, timestamps, float(first[k]), float(first[k]), b"", b""))
        else:
            rows.append((1, start, start + (length - 1) * delta, timestamps, float(first[k]), float(last[k]),
                         bytes([0]) if decreasing[k] else b"", b""))
    simple = sc.simple_batch(types, starts, lengths, deltas, first, last, decreasing)
    _same_columns(simple, SegmentBatch.from_rows(rows))
    assert np.array_equal(sc.segment_lengths(simple), lengths)
    # a whole tier A pair at small parameters: compressed chunks (out-of-line payloads) joined and reordered
    for batch in sc.tier_a_batches(**sc.TIER_A_SMALL):
        assert batch.identical(SegmentBatch.from_rows(batch.rows()))
        assert ora.grid_count(batch) == int(sc.segment_lengths(batch).sum())
    parts = [simple.take(np.arange(40)), sc.tier_a_batches(**sc.TIER_A_SMALL)[0], simple.take(np.arange(40, 90))]
    joined = sc.concat_batches(parts)  # (the items; SegmentBatch.concat packs the payloads of a reordered batch anew)
    assert joined.identical(SegmentBatch.concat(parts)) and joined.identical(SegmentBatch.from_rows(joined.rows()))
    packed = SegmentBatch.from_rows(parts[1].rows()[:500])  # (payloads in row order: the views come out the same too)
    _same_columns(sc.concat_batches([packed, simple]), SegmentBatch.concat([packed, simple]))


def test_packed_mask_equals_packbits_at_every_bit_position():
    n_rows = 64 * 6 + 37
    for begin in range(64):
        for length in [1, 63, 64, 65, 129] + [k - begin for k in range(begin + 1, begin + 65)]:
            bits = np.zeros(n_rows, dtype=bool)
            bits[5] = True  # (what is there already stays)
            bits[begin:begin + length] = True
            for by_run in (True, False):
                mask = sc.PackedMask(n_rows)
                mask.set_bits(5, [True])
                if by_run:
                    mask.set_run(begin, length)
                else:
                    mask.set_bits(begin, np.ones(length, dtype=bool))
                assert np.array_equal(mask.bytes, sc.pack_bits(bits)), (begin, length, by_run)
                assert mask.count() == int(bits.sum()) and mask.count_run(begin, length) == length
                assert mask.count_run(3, begin + 9) == int(bits[3:begin + 12].sum())
                assert np.array_equal(mask.get_bits(begin, length), bits[begin:begin + length])
                assert np.array_equal(mask.get_bits(max(begin - 3, 0), 70), bits[max(begin - 3, 0):max(begin - 3, 0) + 70])
    rng = np.random.default_rng(3)
    bits = rng.random(n_rows) < 0.3
    mask = sc.PackedMask(n_rows)
    for at in range(0, n_rows, 29):
        mask.set_bits(at, bits[at:at + 29])
    assert np.array_equal(mask.bytes, sc.pack_bits(bits))


def _small_tier_c():
    batches = sc.tier_c_batches(**sc.TIER_C_SMALL)
    return batches, [sc.Field(batch) for batch in batches], [sc.Streamed(batch) for batch in batches]


def _same_agg(got, expected, what):
    """Count, min and max bit for bit; the sums are the same additions in f64 in another order (per segment, then
    merged, against one pairwise sum over the grid): equal to within 1e-13 of the sum of magnitudes (a few thousand
    additions of relative error 2^-53 each)."""
    assert got[0] == expected[0], what
    assert np.float32(got[2]).view(np.uint32) == np.float32(expected[2]).view(np.uint32), what
    assert np.float32(got[3]).view(np.uint32) == np.float32(expected[3]).view(np.uint32), what
    assert abs(got[1] - expected[1]) <= 1e-13 * max(expected[4], 1e-300), (what, got[1], expected[1])
    assert abs(got[4] - expected[4]) <= 1e-13 * max(expected[4], 1e-300), what


def test_the_closed_form_and_streaming_paths_equal_the_oracle_grid():
    batches, fields, streams = _small_tier_c()
    assert np.array_equal(fields[0].ts, fields[1].ts) and len(batches[0]) != len(batches[1])
    first, last = int(fields[0].ts[0]), int(fields[0].ts[-1])
    middle = (first + (last - first) // 5 + 3, last - (last - first) // 4 - 1)
    giant_end = int(batches[0].end_time[sc.TIER_C_SMALL["n_giants"] - 1])
    ranges = [(sc.I64_MIN, sc.I64_MAX), middle, (first + 1005, giant_end + 20_000), (last + 5, last + 50)]
    specs = [dict(), dict(lo=0.0), dict(lo=90.0), dict(lo=-20.0, hi=85.0, hi_open=True), dict(lo=1e30)]
    origin, n_buckets = first - 1234, 37
    width = (last - origin) // (n_buckets - 2)
    for f, (field, streamed) in enumerate(zip(fields, streams)):
        assert np.array_equal(streamed.lengths, field.rows)
        assert streamed.closed.sum() >= sc.TIER_C_SMALL["n_giants"] * 0.6 and not streamed.closed.all()
        for t_lo, t_hi in ranges:
            inside = field.in_range(t_lo, t_hi)
            rows, first_row = streamed.rows(t_lo, t_hi)
            assert np.array_equal(rows, np.bincount(field.segment[inside], minlength=len(field.batch)))
            for spec in specs:
                flt = mdb.value_filter(t_lo=t_lo, t_hi=t_hi, **spec)
                got = sc.streamed_filter(streamed, flt, origin, width, n_buckets, want_rows=True)
                keep = sc.passes(field.keys[inside], flt)
                what = (f, t_lo, spec)
                assert got["n_rows"] == int(inside.sum()) and got["mask"].count() == int(keep.sum()), what
                assert np.array_equal(got["mask"].bytes, sc.pack_bits(keep)), what
                _same_agg(got["agg"], sc.expected_agg(field.values[inside][keep]), what)
                assert np.array_equal(got["ts"], field.ts[inside][keep]), what
                assert np.array_equal(got["values"].view(np.uint32), field.values[inside][keep].view(np.uint32)), what
                assert np.array_equal(got["rows_per_segment"],
                                      np.bincount(field.segment[inside][keep], minlength=len(field.batch))), what
                cells = sc.Cells(field.ts, field.values, field.segment, np.zeros(len(field.batch), dtype=np.uint32), 1,
                                 origin, width, n_buckets)
                full = np.zeros(len(field.ts), dtype=bool)
                full[inside] = keep
                expected, magnitude = cells.expected(full)
                assert np.array_equal(got["cells"][0]["count"], expected["count"]), what
                for name in ("min", "max"):
                    assert np.array_equal(got["cells"][0][name].view(np.uint32), expected[name].view(np.uint32)), (what, name)
                assert np.all(np.abs(got["cells"][0]["sum"] - expected["sum"]) <= 1e-13 * np.maximum(magnitude, 1e-300)), what
                # the other field's rows under this mask
                other, other_stream = fields[1 - f], streams[1 - f]
                total, selected = sc.streamed_under_mask(other_stream, got["mask"], t_lo, t_hi)
                _same_agg(total, sc.expected_agg(other.values[inside][keep]), what)
                assert np.array_equal(selected, np.bincount(other.segment[inside][keep], minlength=len(other.batch))), what
        picked = np.unique(np.random.default_rng(4).integers(0, len(field.ts), 500))
        ts, values, segment = sc.streamed_rows_at(streamed, field.first_row, picked)
        assert np.array_equal(ts, field.ts[picked]) and np.array_equal(segment, field.segment[picked])
        assert np.array_equal(values.view(np.uint32), field.values[picked].view(np.uint32))


def test_cells_equal_a_plain_loop():
    batch = sc.tier_a_batches(**sc.TIER_A_SMALL)[0]
    field = sc.Field(batch)
    groups = (np.arange(len(batch)) % 3).astype(np.uint32)
    origin, n_buckets = int(field.ts[0]) + 1000, 11
    width = (int(field.ts[-1]) - origin) // 12
    cells = sc.Cells(field.ts, field.values, field.segment, groups, 3, origin, width, n_buckets)
    keep = field.values > 0
    expected, magnitude = cells.expected(keep)
    for g in range(3):
        for b in range(n_buckets):
            here = keep & (groups[field.segment] == g) & ((field.ts - origin) // width == b)
            count, total, low, high, size = sc.expected_agg(field.values[here])
            assert expected[g, b]["count"] == count and expected[g, b]["min"] == low and expected[g, b]["max"] == high
            assert abs(expected[g, b]["sum"] - total) <= 1e-13 * max(size, 1e-300) and abs(magnitude[g, b] - size) <= 1e-13 * max(size, 1e-300)


# ---- the tiers at full parameters: their preconditions from the metadata ----------------------------------------------

def _rows_of(batches):
    lengths = [sc.segment_lengths(batch) for batch in batches]
    assert len({int(n.sum()) for n in lengths}) == 1  # (the fields line up in their row count)
    for batch, n in zip(batches[:1], lengths[:1]):
        assert ora.grid_count(batch) == int(n.sum())
    return lengths


def test_tier_a_meets_its_preconditions():
    batches = sc.tier_a_batches(**sc.TIER_A)
    lengths = _rows_of(batches)
    rows = int(lengths[0].sum())
    assert len(batches[0]) > 1_048_576 and len(batches[1]) > len(batches[0])
    assert rows > 33_554_432 and mdb.mask_words(rows) > 524_288 and rows % 64 != 0
    for batch in batches:
        assert set(batch.model_type_id.tolist()) == {sc.PMC, sc.SWING, sc.MACAQUE}
    assert (batches[0].residuals.lengths() > 0).sum() > 1000 and sc.per_point_segments(batches[0]).sum() > 2000
    assert lengths[0].min() == 1 and lengths[0].max() > 640
    assert (np.diff(batches[0].start_time) > 0).all()


def test_tier_b_meets_its_preconditions():
    batches = sc.tier_b_batches(**sc.TIER_B)
    lengths = _rows_of(batches)
    for batch, n in zip(batches, lengths):
        per_point = sc.per_point_segments(batch)
        rows = n[per_point]
        assert int(rows.sum()) > 3 * (1 << 24) and int(per_point.sum()) >= 40_000
        # the slices of at most 2^24 points, cut as the library cuts them: the first holds more than 32 768 segments
        assert int(np.searchsorted(np.cumsum(rows), 1 << 24, side="right")) > 32_768
    assert ((batches[0].residuals.lengths() > 0) & (batches[0].model_type_id != sc.MACAQUE)).sum() > 1000
    assert (batches[0].model_type_id == sc.MACAQUE).sum() >= 40_000


def test_tier_c_meets_its_preconditions():
    batches = sc.tier_c_batches(**sc.TIER_C)
    lengths = _rows_of(batches)
    n_giants = sc.TIER_C["n_giants"]
    for batch, n, giants in zip(batches, lengths, (n_giants, n_giants + 1)):
        assert int(n[:giants].sum()) > (1 << 32)  # the tail's first row
        assert n.max() <= 1_000_000 and int(n.sum()) % 64 != 0
        assert (batch.timestamps.lengths()[:giants] == 3).all()
        assert np.array_equal(batch.start_time[1:giants], batch.end_time[:giants - 1] + sc.GIANT_DELTA)
        assert 50 < (batch.model_type_id[:giants] == sc.SWING).sum() < 200
        tail = batch.model_type_id[giants:]  # (lossless, the tail of field 0 has no PMC-Mean segment)
        assert {sc.SWING, sc.MACAQUE} <= set(tail.tolist()) and (batch.residuals.lengths()[giants:] > 0).any()
        assert sc.per_point_segments(batch)[giants:].sum() > 10
    assert not np.array_equal(batches[0].start_time[:n_giants], batches[1].start_time[:n_giants])
