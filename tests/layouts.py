"""Physical layouts of the BinaryView columns, for the layout-invariance tests (plain numpy, no GPU).

``relayout(batch, mode, seed)`` gives the timestamps, values and residuals columns of a batch new views and new data
buffers without changing one payload byte: ``batch.identical(relayout(batch, ...))`` holds for every mode. Payloads of
12 bytes or fewer stay inside their views, as Arrow requires. What the suite builds everywhere else is the canonical
layout: one data buffer per column, payloads back to back in row order, the first at byte 0.

``corpus()`` is one batch (a single series with ascending timestamps) with its timestamps and values, built with the
oracle's compressor; ``corpus_conditions`` asserts what the tests rely on it to hold.
"""

import functools

import numpy as np

import cases
import oracle_lib as ora
import modelardb_rs_amd as mdb

MODES = ("padded-one", "three", "empty-first", "blocks", "shared", "odd-base")
COLUMNS = ("timestamps", "values", "residuals")
FILLER = 0xFF          # never zero: a reader that uses a bit beyond its payload gets a wrong answer, not a lucky one
MAX_FILLER = 17        # 0..17 bytes in front of a payload
FIRST_BLOCK, LARGEST_BLOCK = 64, 2 << 20   # arrow's view builder starts at 8 KiB; scaled down for this corpus


def _inline_view(view, item):
    view[0:4] = np.frombuffer(np.int32(len(item)).tobytes(), dtype=np.uint8)
    view[4:4 + len(item)] = np.frombuffer(item, dtype=np.uint8)


def _reference_view(view, item, buffer_index, offset):
    view[0:4] = np.frombuffer(np.int32(len(item)).tobytes(), dtype=np.uint8)
    view[4:8] = np.frombuffer(item[:4], dtype=np.uint8)
    view[8:12] = np.frombuffer(np.int32(buffer_index).tobytes(), dtype=np.uint8)
    view[12:16] = np.frombuffer(np.int32(offset).tobytes(), dtype=np.uint8)


def _padded(items, rows, mode, rng):
    """[(row, buffer index, offset)] and the buffers: the out-of-line payloads of `rows` in shuffled order, dealt over
    the mode's buffers, each behind 0..17 filler bytes; per buffer the first begins at byte 0 (the next fifteen at
    offsets 1..15 mod 16) and the last ends at the buffer's last byte."""
    n_buffers = {"padded-one": 1, "three": 3, "empty-first": 3, "shared": 2, "odd-base": 3}[mode]
    usable = list(range(1, n_buffers)) if mode == "empty-first" else list(range(n_buffers))
    order = [rows[k] for k in rng.permutation(len(rows))]
    data = [bytearray() for _ in range(n_buffers)]
    placed_in = [0] * n_buffers
    places, copies = [], {}
    for k, row in enumerate(order):
        item = items[row]
        if mode == "shared" and item in copies:
            places.append((row,) + copies[item])
            continue
        # (every usable buffer gets a payload before the dice decide)
        b = usable[k] if k < len(usable) else usable[int(rng.integers(len(usable)))]
        if placed_in[b] == 0:
            filler = 0
        elif placed_in[b] < 16:
            filler = (placed_in[b] - len(data[b])) % 16
        else:
            filler = int(rng.integers(MAX_FILLER + 1))
        data[b] += bytes([FILLER]) * filler
        places.append((row, b, len(data[b])))
        copies[item] = (b, len(data[b]))
        data[b] += item
        placed_in[b] += 1
    buffers = []
    for b in range(n_buffers):
        if mode == "odd-base":
            # a slice of a larger array: the base address is not a multiple of 16
            backing = np.full(len(data[b]) + 32, FILLER, dtype=np.uint8)
            k = int(rng.integers(1, 16))
            k += 1 if (backing.ctypes.data + k) % 16 == 0 else 0
            buffer = backing[k:k + len(data[b])]
            buffer[:] = np.frombuffer(bytes(data[b]), dtype=np.uint8)
            assert len(buffer) == 0 or buffer.ctypes.data % 16 != 0
        else:
            buffer = np.frombuffer(bytes(data[b]), dtype=np.uint8)
        buffers.append(buffer)
    return places, buffers


def _blocks(items, rows):
    """Arrow's view builder: row order kept, payloads appended to blocks of 64, 128, ... bytes (at most 2 MiB); one that
    does not fit opens the next block, one larger than that block gets a buffer of its own."""
    places, buffers = [], []
    block, capacity, next_size = bytearray(), FIRST_BLOCK, FIRST_BLOCK

    def flush():
        if block:
            buffers.append(np.frombuffer(bytes(block), dtype=np.uint8))

    for row in rows:
        item = items[row]
        if len(block) + len(item) > capacity:
            flush()
            next_size = min(2 * next_size, LARGEST_BLOCK)
            block, capacity = bytearray(), max(next_size, len(item))
        places.append((row, len(buffers), len(block)))
        block += item
    flush()
    return places, buffers


def relayout_column(column, mode, rng):
    if mode not in MODES:
        raise ValueError(f"unknown layout mode {mode!r}")
    items = column.to_bytes_list()
    views = np.zeros((len(items), 16), dtype=np.uint8)
    rows = []
    for row, item in enumerate(items):
        if len(item) <= 12:
            _inline_view(views[row], item)
        else:
            rows.append(row)
    places, buffers = _blocks(items, rows) if mode == "blocks" else _padded(items, rows, mode, rng)
    for row, buffer_index, offset in places:
        _reference_view(views[row], items[row], buffer_index, offset)
    return mdb.BinaryViewColumn(views, buffers)


def relayout(batch, mode, seed):
    """`batch` with the three BinaryView columns laid out anew (see the module's docstring and MODES)."""
    columns = [relayout_column(getattr(batch, name), mode, np.random.default_rng([seed, MODES.index(mode), c]))
               for c, name in enumerate(COLUMNS)]
    return mdb.SegmentBatch(batch.model_type_id.copy(), batch.start_time.copy(), batch.end_time.copy(), columns[0],
                            batch.min_value.copy(), batch.max_value.copy(), columns[1], columns[2], batch.error.copy(),
                            None if batch.chunk_index is None else batch.chunk_index.copy())


def part_cuts(n):
    """The row bounds of the three parts of a batch of n rows."""
    return [0, n // 3 + 1, (2 * n) // 3 + 2, n]


def cut(batch):
    """The batch cut at part_cuts, every part in the layout it had."""
    cuts = part_cuts(len(batch))
    return [batch.slice(cuts[k], cuts[k + 1]) for k in range(3)]


def three_parts(batch, mode, seed):
    """The batch cut at two rows, every part laid out again in a mode of its own: what a `_list` entry point or one
    grid_submit ticket is handed. One part brings one buffer per column (`padded-one`; two, `shared`, where the whole
    is `padded-one` itself), one three (`odd-base`; `empty-first` where the whole is `odd-base`) and one arrow's blocks,
    about ten (under a whole in `blocks` too: a part's blocks begin at 64 bytes again), so the joint table shifts the
    later parts' buffer indexes unevenly. Which part gets which turns with the mode."""
    cuts = part_cuts(len(batch))
    modes = ["shared" if mode == "padded-one" else "padded-one", "empty-first" if mode == "odd-base" else "odd-base",
             "blocks"]
    turn = MODES.index(mode) % 3
    modes = modes[turn:] + modes[:turn]
    return [relayout(batch.slice(cuts[k], cuts[k + 1]), modes[k], seed + 1 + k) for k in range(3)]


def groups_of_parts(groups):
    """One group id per row of a batch, cut as `cut` and `three_parts` cut the batch."""
    cuts = part_cuts(len(groups))
    return [groups[cuts[k]:cuts[k + 1]] for k in range(3)]


def halves(batch):
    """The batch in two parts, cut at a row that is none of part_cuts': what the second list of an operator on two
    fields is handed, so that the two lists are cut at different rows."""
    middle = len(batch) // 2 + 3
    return [batch.slice(0, middle), batch.slice(middle, len(batch))]


def out_of_line_offsets(column):
    """(buffer index, offset) of every out-of-line view, as two arrays."""
    words = column.views.view(np.int32).reshape(-1, 4)
    out = words[:, 0] > 12
    return words[out, 2], words[out, 3]


# ---- the corpus -----------------------------------------------------------------------------------------------------

TAIL_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200, 255, 256, 300)
NOISE_LENGTHS = (3, 70, 300, 1000, 1024, 1025, 4096, 4097, 9000)


def _series(synthetic_length):
    """[(timestamps from 0 on, values, error bound)]"""
    bounds = cases.error_bounds()
    rng = np.random.default_rng(2906)
    out = []
    for k, (eb_name, irregular) in enumerate((("lossless", True), ("abs0.01", False), ("rel5", True), ("rel1", False))):
        timestamps, values = cases.synthetic_series(synthetic_length, irregular, (1.0, 1.05), 800 + k)
        out.append((timestamps, values, bounds[eb_name]))
    out += [(timestamps, values, cases.LOSSLESS) for _, timestamps, values in cases.edge_case_series()]
    tails = {}                  # (the residual tails of test_resident_batches_are_decoded_piece_by_piece)
    for n_res in TAIL_LENGTHS:
        values = np.concatenate([np.full(20, 5.0, dtype=np.float32), rng.uniform(-1e30, 1e30, n_res).astype(np.float32),
                                 np.arange(20, dtype=np.float32) * 3 + 1])
        tails[n_res] = (np.arange(len(values), dtype=np.int64) * 100, values, cases.LOSSLESS)
    noise = {}                  # (every value opens a new window: MacaqueV streams of n values)
    for n in NOISE_LENGTHS:
        noise[n] = (np.arange(n, dtype=np.int64) * 100, rng.uniform(-1e3, 1e3, n).astype(np.float32), cases.LOSSLESS)
    out += list(tails.values()) + list(noise.values())
    out.append((np.cumsum(rng.integers(1, 400, 5000)).astype(np.int64), rng.uniform(-1e3, 1e3, 5000).astype(np.float32),
                cases.LOSSLESS))
    # Three series once more: rows with EQUAL payload bytes in every column, which the "shared" mode points at one
    # copy (without them the corpus has no two equal out-of-line payloads).
    irregular = (np.cumsum(rng.integers(1, 400, 300)).astype(np.int64), rng.uniform(-1e3, 1e3, 300).astype(np.float32),
                 cases.LOSSLESS)
    out += [irregular, tails[65], noise[1025], irregular]
    return out


@functools.lru_cache(maxsize=None)
def corpus(synthetic_length=20_000):
    """(batch, timestamps, values): one series with ascending timestamps in the canonical layout - every series of
    _series() shifted behind the one before it."""
    parts, all_timestamps, all_values = [], [], []
    begin = 1_000
    for timestamps, values, eb in _series(synthetic_length):
        timestamps = np.asarray(timestamps, dtype=np.int64)
        timestamps = timestamps - timestamps[0] + begin
        parts.append(ora.try_compress_univariate_time_series(timestamps, values, eb))
        all_timestamps.append(timestamps)
        all_values.append(np.asarray(values, dtype=np.float32))
        begin = int(timestamps[-1]) + 700
    return mdb.SegmentBatch.concat(parts), np.concatenate(all_timestamps), np.concatenate(all_values)


def macaque_v_lengths(batch):
    """The number of values of every MacaqueV segment (the residual tails are not counted)."""
    rows = np.flatnonzero(batch.model_type_id == mdb.MDB_MACAQUE_V_ID)
    timestamps = batch.timestamps.to_bytes_list()
    residuals = batch.residuals.to_bytes_list()   # (the last byte of a residual payload is its number of values)
    return np.array([ora.seg_len(int(batch.start_time[r]), int(batch.end_time[r]), timestamps[r])
                     - (residuals[r][-1] if residuals[r] else 0) for r in rows], dtype=np.int64)


def corpus_conditions(batch, seeds=(0, 1)):
    """What the layout tests rely on the corpus to hold: conditions, not measurements."""
    for name in COLUMNS:
        lengths = getattr(batch, name).lengths()
        assert int((lengths > 12).sum()) >= 64, name
        assert int(((lengths > 0) & (lengths <= 12)).sum()) >= 16, name
    lengths = macaque_v_lengths(batch)
    assert int((lengths >= 4097).sum()) >= 3     # more than one wave of 64-value pieces, and a "long" chain
    assert int((lengths > 64).sum()) >= 8
    assert np.all(np.diff(batch.start_time) > 0) and np.all(batch.end_time >= batch.start_time)
    for name in COLUMNS:   # (rows for the "shared" mode to share)
        payloads = [item for item in getattr(batch, name).to_bytes_list() if len(item) > 12]
        assert len(set(payloads)) < len(payloads), name
    for seed in seeds:
        for mode in MODES:
            relaid = relayout(batch, mode, seed)
            for name in COLUMNS:
                column = getattr(relaid, name)
                if mode == "padded-one":
                    assert len(column.buffers) == 1
                    _, offsets = out_of_line_offsets(column)
                    assert len(np.unique(offsets % 16)) == 16, (name, seed)
                else:
                    assert len(column.buffers) >= 2, (mode, name, seed)
