"""What the resident-state tests share: two corpora, a table of operators, orders and switch schedules (no GPU needed
to import).

A batch that stays on the device keeps what its calls found out about it (cursors, walks, per-segment totals, failure
flags: MvIndex in csrc/mdb_common.hpp). tests/test_gpu_resident_state.py asks that a call's answer never depends on
what was kept: here are the calls (OPERATORS: every one a function (context, resident, corpus) -> the digest of all it
returned), the orders to make them in (`williams`), the switch settings to make them under (SETTINGS, `switch_schedules`)
and the batches (`corpus_a`, `corpus_b`, `corpus_plain`) with what the calls are asked about each (`Corpus`).
"""

import ctypes
import functools
import hashlib

import numpy as np

import cases
import layouts
import oracle_lib as ora
import modelardb_rs_amd as mdb
from modelardb_rs_amd import MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM

ALL = MDB_AGG_COUNT | MDB_AGG_MIN | MDB_AGG_MAX | MDB_AGG_SUM
QUANTILES = (0.0, 0.5, 0.999, 1.0)
N_EDGES = 64
N_GROUPS = 2


# ---- digests ----------------------------------------------------------------------------------------------------------

def _feed(hasher, item):
    if item is None:
        hasher.update(b"<none>")
    elif isinstance(item, (bytes, bytearray)):
        hasher.update(b"<bytes %d>" % len(item))
        hasher.update(item)
    elif isinstance(item, np.ndarray):
        hasher.update(f"<array {item.dtype.str} {item.shape}>".encode())
        hasher.update(np.ascontiguousarray(item).tobytes())
    elif isinstance(item, ctypes.Structure):
        hasher.update(f"<struct {type(item).__name__}>".encode())
        hasher.update(ctypes.string_at(ctypes.addressof(item), ctypes.sizeof(item)))
    elif isinstance(item, (bool, int, np.integer)):
        hasher.update(f"<int {int(item)}>".encode())
    elif isinstance(item, dict):
        hasher.update(b"<dict %d>" % len(item))
        for key in sorted(item):
            hasher.update(str(key).encode())
            _feed(hasher, item[key])
    elif isinstance(item, (tuple, list)):
        hasher.update(b"<list %d>" % len(item))
        for member in item:
            _feed(hasher, member)
    else:  # (a float would have to be rounded to be written down: hand its bits over as an array or a struct)
        raise TypeError(f"no digest of a {type(item).__name__}")


def digest(*items):
    """The SHA-256 of what a call returned: arrays by dtype, shape and bytes (bit patterns: -0.0 is not 0.0, a NaN
    keeps its payload), C structs by their bytes, integers by value, None, and dicts, tuples and lists of these."""
    hasher = hashlib.sha256()
    _feed(hasher, items)
    return hasher.digest()


# ---- the corpora ------------------------------------------------------------------------------------------------------

def _keys(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def _floats_of_keys(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return (keys ^ ((keys >> 31) & 0x7FFFFFFF)).astype(np.int32).view(np.float32)


class Corpus:
    """One batch with its series, and what the operators ask about it: two time ranges, three value filters, the
    histogram's edges, the buckets and the groups (the kinds tests/test_gpu_layouts.py uses on the same corpus)."""

    def __init__(self, name, batch, timestamps, values):
        self.name, self.batch, self.timestamps, self.values = name, batch, timestamps, values
        n = len(batch)
        lengths = layouts.macaque_v_lengths(batch)
        long_rows = np.flatnonzero(batch.model_type_id == mdb.MDB_MACAQUE_V_ID)[lengths >= 4097]
        assert len(long_rows) >= 3
        self.long_rows = long_rows
        start, end = batch.start_time[long_rows].tolist(), batch.end_time[long_rows].tolist()
        # from inside a segment with irregular timestamps in front to the middle of the third long MacaqueV stream
        self.cut_range = (int(timestamps[len(timestamps) // 7]), start[2] + (end[2] - start[2]) // 2)
        # from the first point of one segment to the last of another: whole segments only
        self.whole_range = (int(batch.start_time[n // 5]), int(batch.end_time[(4 * n) // 5]))
        # from inside the first long stream to inside the second
        self.inner_range = (start[0] + 100_001, end[1] - 33_301)
        self.band = mdb.value_filter(lo=130.0, hi=160.0, hi_open=True)
        self.bounded = mdb.value_filter(lo=-500.0, hi=500.0, lo_open=True, t_lo=self.inner_range[0], t_hi=self.inner_range[1])
        self.groups = (np.arange(n) % N_GROUPS).astype(np.uint32)
        self.buckets = (int(timestamps[0]) - 7, 777_777, 40)  # origin, width, number: under cut_range
        keys = _keys(values)
        lo, hi = int(keys.min()), int(keys.max())
        picked = np.unique(np.linspace(lo, hi, N_EDGES + 2)[1:-1].astype(np.int64))
        self.edges = _floats_of_keys(picked[(picked > lo) & (picked <= hi)])
        assert len(self.edges) == N_EDGES

    def rows_inside(self, t_lo, t_hi):
        return int(((self.timestamps >= t_lo) & (self.timestamps <= t_hi)).sum())


def _fitted(factor, keep=None):
    parts, all_timestamps, all_values = [], [], []
    begin = 1_000
    for timestamps, values, eb in layouts._series(20_000):   # (layouts.corpus(), with the values scaled)
        if keep is not None and not keep(np.asarray(values, dtype=np.float32)):
            continue
        timestamps = np.asarray(timestamps, dtype=np.int64)
        timestamps = timestamps - timestamps[0] + begin
        values = (np.asarray(values, dtype=np.float32) * np.float32(factor)).astype(np.float32)
        parts.append(ora.try_compress_univariate_time_series(timestamps, values, eb))
        all_timestamps.append(timestamps)
        all_values.append(values)
        begin = int(timestamps[-1]) + 700
    return mdb.SegmentBatch.concat(parts), all_timestamps, all_values


@functools.lru_cache(maxsize=None)
def corpus_a():
    """layouts.corpus() as it stands."""
    return Corpus("corpus", *layouts.corpus())


@functools.lru_cache(maxsize=None)
def corpus_b():
    """The same series with every value multiplied by 1.5 before fitting: the same kind of content, other answers."""
    with np.errstate(over="ignore", invalid="ignore"):
        batch, timestamps, values = _fitted(1.5)
    return Corpus("corpus_b", batch, np.concatenate(timestamps), np.concatenate(values))


PLAIN_BELOW = 1e9


@functools.lru_cache(maxsize=None)
def corpus_plain():
    """The series of the corpus whose values are all finite and below PLAIN_BELOW in size. The corpus itself holds NaN,
    -inf and +inf, so its SUM over the whole batch is NaN whatever a segment adds to it, and its tails of +-1e30 would
    swallow a segment's sum in the total's rounding: there a wrong kept per-segment sum (MvIndex::agg_walk_sums) cannot
    show. Here every segment's sum shows in the bits of the total (`plain_conditions`)."""
    batch, timestamps, values = _fitted(1.0, keep=lambda v: bool(np.isfinite(v).all() and np.abs(v).max() < PLAIN_BELOW))
    return Corpus("corpus_plain", batch, np.concatenate(timestamps), np.concatenate(values))


def plain_conditions(corpus):
    """corpus_conditions, and: SUM over the whole batch is finite, and the points of every Swing or PMC-Mean segment
    with irregular timestamps - the ones whose sums a resident batch keeps - add up to more than 16 units in the last
    place of that total, so that losing or doubling any of them changes it."""
    corpus_conditions(corpus)
    batch = corpus.batch
    total = ora.agg_batch(batch, ALL).sum
    assert np.isfinite(total) and total != 0
    _, values, lengths = ora.grid_batch(batch)[:3]
    ends = np.cumsum(lengths.astype(np.int64))
    sums = np.add.reduceat(np.asarray(values, dtype=np.float64), ends - lengths.astype(np.int64))
    walked = irregular_rows(batch) & (batch.model_type_id != mdb.MDB_MACAQUE_V_ID)
    assert int(walked.sum()) >= 16
    assert np.all(np.abs(sums[walked]) > 16 * np.spacing(abs(total)))


@functools.lru_cache(maxsize=None)
def series_b():
    """(timestamps, values, chunk offsets) of corpus_b's series, one chunk per series: what a fit on the device takes."""
    with np.errstate(over="ignore", invalid="ignore"):
        _, timestamps, values = _fitted(1.5)
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in values])]).astype(np.uint64)
    return np.concatenate(timestamps), np.concatenate(values), offsets


def irregular_rows(batch):
    """The rows whose timestamps are a delta-of-delta stream (not the start, the end and a count)."""
    return np.array([not ora.are_compressed_timestamps_regular(payload) for payload in batch.timestamps.to_bytes_list()])


def corpus_conditions(corpus):
    """What the resident-state tests rely on a corpus to hold: conditions, not measurements."""
    batch = corpus.batch
    assert int((batch.timestamps.lengths() > 12).sum()) >= 16     # timestamp payloads out of line
    lengths = layouts.macaque_v_lengths(batch)
    assert int((lengths >= 1025).sum()) >= 3                      # the parallel decoder's, and "long" chains
    assert int(((lengths >= 128) & (lengths <= 1024)).sum()) >= 8  # "short" chains of two pieces or more
    irregular = irregular_rows(batch)
    assert int((irregular & (batch.model_type_id == mdb.MDB_SWING_ID)).sum()) >= 1
    assert np.all(np.diff(batch.start_time) > 0) and np.all(batch.end_time[:-1] < batch.start_time[1:])
    # cut_range begins inside a segment with irregular timestamps, ends inside a MacaqueV stream and holds whole
    # segments of both kinds between
    lo, hi = corpus.cut_range
    cut_lo = (batch.start_time < lo) & (batch.end_time >= lo)
    cut_hi = (batch.start_time <= hi) & (batch.end_time > hi)
    assert int((cut_lo & irregular).sum()) == 1 and int((cut_hi & (batch.model_type_id == mdb.MDB_MACAQUE_V_ID)).sum()) == 1
    inside = (batch.start_time >= lo) & (batch.end_time <= hi)
    assert int((inside & irregular).sum()) >= 8 and int((inside & (batch.model_type_id == mdb.MDB_MACAQUE_V_ID)).sum()) >= 8
    # whole_range cuts no segment and holds many, irregular ones and MacaqueV streams among them
    lo, hi = corpus.whole_range
    outside = (batch.end_time < lo) | (batch.start_time > hi)
    inside = (batch.start_time >= lo) & (batch.end_time <= hi)
    assert np.all(outside | inside) and int(outside.sum()) >= 16
    assert int((inside & irregular).sum()) >= 8 and int((inside & (batch.model_type_id == mdb.MDB_MACAQUE_V_ID)).sum()) >= 8
    # inner_range begins and ends inside long MacaqueV streams
    lo, hi = corpus.inner_range
    for bound in (lo, hi):
        row = np.flatnonzero((batch.start_time < bound) & (batch.end_time > bound))
        assert len(row) == 1 and row[0] in corpus.long_rows
    for lo, hi in (corpus.cut_range, corpus.whole_range, corpus.inner_range):
        assert 64 < corpus.rows_inside(lo, hi) < len(corpus.timestamps)
    # the filters pass some points and not all, the buckets hold points
    band = (corpus.values >= np.float32(130.0)) & (corpus.values < np.float32(160.0))
    assert 64 < int(band.sum()) < len(corpus.values) - 64
    origin, width, n_buckets = corpus.buckets
    buckets = (corpus.timestamps - origin) // width
    keep = (buckets >= 0) & (buckets < n_buckets) & (corpus.timestamps >= corpus.cut_range[0]) & (corpus.timestamps <= corpus.cut_range[1])
    assert len(np.unique(buckets[keep])) >= 4
    assert np.all(np.diff(_keys(corpus.edges)) > 0)


# ---- the operators ----------------------------------------------------------------------------------------------------
# (context, resident, corpus) -> digest. Only the forms that take a batch on the device.

def _grid_whole(context, resident, corpus):
    return digest(*context.grid_resident(resident))


def _grid_range(context, resident, corpus):
    return digest(*context.grid_resident(resident, corpus.cut_range))


def _agg(which):
    def run(context, resident, corpus):
        return digest(context.agg_batch_dev(resident, which))
    return run


def _agg_range_cut(context, resident, corpus):
    return digest(context.agg_batch_range_dev(resident, *corpus.cut_range, ALL))


def _agg_range_whole(context, resident, corpus):
    return digest(context.agg_batch_range_dev(resident, *corpus.whole_range, ALL))


def _agg_buckets(context, resident, corpus):
    origin, width, n_buckets = corpus.buckets
    return digest(context.agg_buckets_dev(resident, origin, width, n_buckets, corpus.groups, t_lo=corpus.cut_range[0],
                                          t_hi=corpus.cut_range[1], n_groups=N_GROUPS))


def _agg_filter(context, resident, corpus):
    return digest(context.agg_filter_dev(resident, corpus.band, ALL))


def _grid_filter(context, resident, corpus):
    return digest(*context.grid_filter_resident(resident, corpus.bounded))


def _mask_then_agg(context, resident, corpus):
    flt = corpus.bounded
    n_rows = corpus.rows_inside(flt.t_lo, flt.t_hi)
    words = mdb.mask_words(n_rows)
    mask = context.upload_array(np.full((words + 1) * 8, 0xFF, dtype=np.uint8))  # (one guard word behind)
    try:
        counts = context.mask_filter_dev(resident, flt, mask, words)
        bits = context.download_mask(mask, n_rows, with_padding=True)
        guard = context.download_array(mask, 8, np.uint8, offset_elements=words * 8)
        state = context.agg_mask_dev(resident, flt.t_lo, flt.t_hi, mask, n_rows, ALL)
    finally:
        context.dev_free(mask)
    return digest(counts, bits, guard, state)


def _agg_buckets_filter(context, resident, corpus):
    origin, width, n_buckets = corpus.buckets
    return digest(context.agg_buckets_filter_dev(resident, corpus.band, origin, width, n_buckets, corpus.groups,
                                                 t_lo=corpus.cut_range[0], t_hi=corpus.cut_range[1], n_groups=N_GROUPS))


def _hist(context, resident, corpus):
    return digest(context.hist_dev(resident, corpus.edges, corpus.groups, n_groups=N_GROUPS))


def _quantile(context, resident, corpus):
    lo, hi, n_points = context.quantile_dev(resident, QUANTILES)
    return digest(lo, hi, n_points)


def batch_digest(batch):
    return digest(batch.model_type_id, batch.start_time, batch.end_time, batch.min_value, batch.max_value,
                  batch.timestamps.to_bytes_list(), batch.values.to_bytes_list(), batch.residuals.to_bytes_list())


def _download(context, resident, corpus):
    return batch_digest(resident.download())


OPERATORS = [
    ("grid", _grid_whole),
    ("grid range", _grid_range),
    ("count", _agg(MDB_AGG_COUNT)),
    ("min max", _agg(MDB_AGG_MIN | MDB_AGG_MAX)),
    ("all four", _agg(ALL)),
    ("sum", _agg(MDB_AGG_SUM)),
    ("range cut", _agg_range_cut),
    ("range whole", _agg_range_whole),
    ("buckets", _agg_buckets),
    ("filter", _agg_filter),
    ("grid filter", _grid_filter),
    ("mask", _mask_then_agg),
    ("buckets filter", _agg_buckets_filter),
    ("hist", _hist),
    ("quantile", _quantile),
    ("download", _download),
]
K = len(OPERATORS)
assert K % 2 == 0 and K >= 14


# ---- orders -----------------------------------------------------------------------------------------------------------

def williams(k):
    """The cyclic Williams design for an even k: k permutations of range(k), row r = [0, 1, k-1, 2, k-2, ...] + r mod k.
    Every member is first once and last once, and every ordered pair (a, b) has b directly after a exactly once."""
    if k % 2 or k < 2:
        raise ValueError("the cyclic Williams design is a single square for an even k only")
    first = [0]
    for step in range(1, k // 2 + 1):
        first.append(step)
        if len(first) < k:
            first.append(k - step)
    return [[(member + r) % k for member in first] for r in range(k)]


# ---- switches ---------------------------------------------------------------------------------------------------------

SWITCHES = ("MDB_GRID_TS_CACHE", "MDB_GRID_TS_JUMPS", "MDB_GRID_MV_INDEX", "MDB_GRID_MV_MIN_VALUES",
            "MDB_AGG_KEEP_CHAIN_OFFSETS", "MDB_AGG_RANGE_PIECES", "MDB_AGG_TS_WALK")
# Switches of other tiers that change which decoder a call takes: unset here.
OTHER_SWITCHES = ("MDB_GRID_MV_HOST_MIN_VALUES", "MDB_SEGMENTS_MERGE_LIMIT", "MDB_FIT_DATA_BUFFER_BYTES")
SETTINGS = {
    "unset": None,
    "ts-cache-0": ("MDB_GRID_TS_CACHE", "0"),
    "ts-jumps-0": ("MDB_GRID_TS_JUMPS", "0"),
    "mv-index-0": ("MDB_GRID_MV_INDEX", "0"),
    "mv-from-8": ("MDB_GRID_MV_MIN_VALUES", "8"),        # (the default is 1024: MV_DEFAULT_MIN_VALUES)
    "mv-from-4096": ("MDB_GRID_MV_MIN_VALUES", "4096"),
    "keep-chains-0": ("MDB_AGG_KEEP_CHAIN_OFFSETS", "0"),
    "range-pieces-0": ("MDB_AGG_RANGE_PIECES", "0"),
    "ts-walk-0": ("MDB_AGG_TS_WALK", "0"),
}
N_SCHEDULES = 6
SCHEDULE_SEED = 1907


def apply_setting(monkeypatch, name):
    """The setting `name` through a pytest MonkeyPatch, every other switch unset."""
    for switch in SWITCHES + OTHER_SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    if SETTINGS[name] is not None:
        monkeypatch.setenv(*SETTINGS[name])


def _circuit(names, rng, start):
    """A closed walk from `start` that takes every ordered pair of different names once (Hierholzer's algorithm on the
    complete digraph, the edges in a seeded order)."""
    out_edges = {a: [b for b in names if b != a] for a in names}
    for a in names:
        rng.shuffle(out_edges[a])
    stack, walk = [start], []
    while stack:
        if out_edges[stack[-1]]:
            stack.append(out_edges[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


@functools.lru_cache(maxsize=None)
def switch_schedules(length=2 * K, n_schedules=N_SCHEDULES):
    """`n_schedules` lists of `length` setting names, fixed by SCHEDULE_SEED. Closed walks over all ordered pairs of
    settings laid end to end and cut so that a schedule begins with the setting the one before ended with: no pair
    of neighbours is lost at a cut, and together the schedules have every setting directly before and directly after
    every other one ("unset" included)."""
    names = list(SETTINGS)
    rng = np.random.default_rng(SCHEDULE_SEED)
    walk = ["unset"]
    while len(walk) < n_schedules * (length - 1) + 1:
        walk += _circuit(names, rng, "unset")[1:]
    return [walk[k * (length - 1): k * (length - 1) + length] for k in range(n_schedules)]


# ---- a malformed stream -----------------------------------------------------------------------------------------------

def malformed(corpus):
    """The corpus plus ONE row: a MacaqueV segment of a few hundred values whose `values` payload is cut to half its
    bytes, everything else as it was (the count the timestamps claim too)."""
    batch = corpus.batch
    lengths = layouts.macaque_v_lengths(batch)
    rows = np.flatnonzero(batch.model_type_id == mdb.MDB_MACAQUE_V_ID)
    residuals = batch.residuals.to_bytes_list()
    picked = [int(r) for r, n in zip(rows, lengths) if 200 <= n <= 400 and not residuals[r]]
    assert picked
    row = list(batch.rows()[picked[0]])
    shift = int(batch.end_time[-1]) + 700 - row[1]   # (behind the last segment: the series stays ascending)
    row[1], row[2] = row[1] + shift, row[2] + shift
    row[6] = row[6][: len(row[6]) // 2]
    return mdb.SegmentBatch.concat([batch, mdb.SegmentBatch.from_rows([tuple(row)])])
