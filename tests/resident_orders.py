"""What the resident-state tests share: two corpora, a table of operators, orders and switch schedules (no GPU needed
to import).

A batch that stays on the device keeps what its calls found out about it (cursors, walks, per-segment totals, failure
flags: MvIndex in csrc/mdb_common.hpp). tests/test_gpu_resident_state.py asks that a call's answer never depends on
what was kept: here are the calls (OPERATORS: every one a function (context, resident, corpus) -> the digest of all it
returned), the orders to make them in (`williams`), the switch settings to make them under (SETTINGS, `switch_schedules`)
and the batches (`corpus_a`, `corpus_b`, `corpus_plain`) with what the calls are asked about each (`Corpus`). Every
batch has a partner - another field of the same series - for the operators that take two; integral, sample and change,
which take no time range, are asked about two runs of buckets, in front of and behind the corpus's gaps of 2^40.
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


SPAN_WIDTH = 20_011    # of the buckets of `Corpus.spans`: no multiple of a sampling interval
SAMPLE_WIDTH = 997     # of the instants of `Corpus.sample_spans`: every run of 1 000 microseconds holds one
LINK_GAP = 500         # the max_gap of the linked operators: above every sampling interval, below the 700 between series
EPISODE_GAP = 150      # the max_gap of the episodes: above the regular interval, inside the irregular ones
GROUP_RUN = 8          # `Corpus.run_groups`: this many neighbouring segments share a group


def spans_of(batch, rear_end, width=SPAN_WIDTH, at_most=5_000):
    """Two runs of buckets (origin, width, n) over a batch of layouts.corpus()'s shape, in front of and behind its gaps
    of 3e9 and twice 2^40 (one run over both would have 1e8 buckets; tests/test_gpu_moments.py's _layout_requests cuts
    there too): the front one over all that lies there, the rear one as far as the bucket that holds `rear_end`."""
    first = int(batch.start_time.min())
    behind = batch.start_time > first + (1 << 41)
    assert 8 <= int(behind.sum()) < len(batch) - 20
    front_last = int(batch.end_time[batch.end_time < first + (1 << 31)].max())   # (not the rows that span the gaps)
    behind_first = int(batch.start_time[behind].min())
    assert behind_first - 33 < rear_end
    spans = ((first - 33, width, (front_last - (first - 33)) // width + 2),
             (behind_first - 33, width, (rear_end - (behind_first - 33)) // width + 1))
    assert all(n_buckets < at_most for _, _, n_buckets in spans), spans
    return spans


class Corpus:
    """One batch with its series, and what the operators ask about it: two time ranges, three value filters, the
    histogram's edges, the buckets and the groups (the kinds tests/test_gpu_layouts.py uses on the same corpus); for
    the operators that take no time range (integral, sample, change) `spans` with `run_groups`; and `partner`, the
    batch of another field of the same series - the same timestamps, cut into segments on its own - for the operators
    that take two (a Corpus, or a function that gives one)."""

    def __init__(self, name, batch, timestamps, values, partner=None):
        self.name, self.batch, self.timestamps, self.values = name, batch, timestamps, values
        self._partner = partner
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
        # Neighbouring segments in one group, so that rows link across segments (under `groups` no two neighbours do),
        # and the buckets and instants of the operators without a time range: they end where cut_range ends.
        self.run_groups = ((np.arange(n) // GROUP_RUN) % N_GROUPS).astype(np.uint32)
        self.spans = spans_of(batch, self.cut_range[1])
        self.sample_spans = spans_of(batch, self.cut_range[1], SAMPLE_WIDTH, at_most=20_000)

    @property
    def partner(self):
        return self._partner() if callable(self._partner) else self._partner

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
    """layouts.corpus() as it stands. Its partner is corpus_b."""
    return Corpus("corpus", *layouts.corpus(), partner=corpus_b)


@functools.lru_cache(maxsize=None)
def corpus_b():
    """The same series with every value multiplied by 1.5 before fitting: the same kind of content, other answers. Its
    partner is the corpus."""
    with np.errstate(over="ignore", invalid="ignore"):
        batch, timestamps, values = _fitted(1.5)
    return Corpus("corpus_b", batch, np.concatenate(timestamps), np.concatenate(values), partner=corpus_a)


PLAIN_BELOW = 1e9


def _plain(values):
    return bool(np.isfinite(values).all() and np.abs(values).max() < PLAIN_BELOW)


@functools.lru_cache(maxsize=None)
def corpus_plain():
    """The series of the corpus whose values are all finite and below PLAIN_BELOW in size. The corpus itself holds NaN,
    -inf and +inf, so its SUM over the whole batch is NaN whatever a segment adds to it, and its tails of +-1e30 would
    swallow a segment's sum in the total's rounding: there a wrong kept per-segment sum (MvIndex::agg_walk_sums) cannot
    show. Here every segment's sum shows in the bits of the total (`plain_conditions`). Its partner: the same series
    times 1.5."""
    batch, timestamps, values = _fitted(1.0, keep=_plain)
    return Corpus("corpus_plain", batch, np.concatenate(timestamps), np.concatenate(values), partner=corpus_plain_b)


@functools.lru_cache(maxsize=None)
def corpus_plain_b():
    """corpus_plain's series (the same `keep`, asked of the values as they are) with every value multiplied by 1.5."""
    batch, timestamps, values = _fitted(1.5, keep=_plain)
    return Corpus("corpus_plain_b", batch, np.concatenate(timestamps), np.concatenate(values), partner=corpus_plain)


def plain_conditions(corpus):
    """corpus_conditions (but for the cell with a NaN or an infinity: there is none here), and: SUM over the whole
    batch is finite, and the points of every Swing or PMC-Mean segment with irregular timestamps - the ones whose sums a
    resident batch keeps - add up to more than 16 units in the last place of that total, so that losing or doubling any
    of them changes it."""
    corpus_conditions(corpus, non_finite=False)
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


def _in_spans(spans, timestamps):
    keep = np.zeros(len(timestamps), dtype=bool)
    for origin, width, n_buckets in spans:
        keep |= (timestamps >= origin) & (timestamps < origin + width * n_buckets)
    return keep


def partner_conditions(corpus):
    """The partner lines up row for row - the oracle's grids of both have the same timestamps - and is cut into
    segments on its own."""
    partner = corpus.partner
    assert partner.partner is corpus
    assert np.array_equal(ora.grid_batch(partner.batch)[0], ora.grid_batch(corpus.batch)[0])
    cuts, partner_cuts = set(corpus.batch.start_time.tolist()), set(partner.batch.start_time.tolist())
    assert len(cuts - partner_cuts) >= 8 and len(partner_cuts - cuts) >= 8
    assert len(partner.groups) == len(partner.batch) and len(partner.edges) == N_EDGES


def span_conditions(corpus, non_finite=True):
    """What `spans` (the buckets of integral and change) and `sample_spans` (the instants of sample) must meet so that
    the three read every kind of row: from the oracle's grid alone. The points of a MacaqueV stream of at least 4097
    values, a residual tail, a Swing segment on irregular timestamps, a cell with a NaN or an infinity (`non_finite`;
    of the instants: one that lies on or between two linked rows of which the earlier is not finite), and links between
    two segments - some that LINK_GAP keeps and some that it cuts - all under `run_groups`. The rear span ends inside
    the last long stream, far in front of the batch's last rows."""
    _spans_conditions(corpus, corpus.spans, SPAN_WIDTH, non_finite, instants=False)
    _spans_conditions(corpus, corpus.sample_spans, SAMPLE_WIDTH, non_finite, instants=True)


def _spans_conditions(corpus, spans, span_width, non_finite, instants):
    batch = corpus.batch
    for origin, width, n_buckets in spans:
        assert width == span_width and n_buckets >= 64
    assert spans[0][0] + spans[0][1] * spans[0][2] < spans[1][0]
    rear_end = spans[1][0] + spans[1][1] * spans[1][2]
    assert int(batch.start_time[corpus.long_rows[2]]) < rear_end < int(batch.end_time[corpus.long_rows[2]])
    timestamps, values, lengths = ora.grid_batch(batch)[:3]
    timestamps = np.asarray(timestamps, dtype=np.int64)
    segment = np.repeat(np.arange(len(batch)), lengths.astype(np.int64))
    inside = _in_spans(spans, timestamps)
    assert 10_000 < int(inside.sum()) < len(timestamps)
    rows_inside = np.bincount(segment[inside], minlength=len(batch))
    # two long streams whole and the one that holds rear_end cut: each with more rows inside than a wave's pieces hold
    assert int((rows_inside[corpus.long_rows] >= 4097).sum()) >= 2
    assert 64 < int(rows_inside[corpus.long_rows[2]]) < int(lengths[corpus.long_rows[2]])
    last_inside = _in_spans(spans, batch.end_time)
    tails = np.array([len(payload) > 0 for payload in batch.residuals.to_bytes_list()])
    assert int((tails & last_inside).sum()) >= 8                                 # (a tail is a segment's last rows)
    swing = irregular_rows(batch) & (batch.model_type_id == mdb.MDB_SWING_ID)
    assert int((swing & (rows_inside > 0)).sum()) >= 8
    if non_finite:
        assert int((~np.isfinite(values) & inside).sum()) >= 8
        assert np.isnan(values[inside]).any() and np.isinf(values[inside]).any()
    if non_finite and instants:
        group = corpus.run_groups.astype(np.int64)[segment]
        gap = np.diff(timestamps)
        linked = (group[1:] == group[:-1]) & (gap > 0) & (gap <= LINK_GAP) & ~np.isfinite(values[:-1])
        hit = 0
        for origin, width, n_instants in spans:
            at = -((origin - timestamps[:-1][linked]) // width)     # the first instant at or behind the earlier row
            hit += int(((at >= 0) & (at < n_instants) & (origin + at * width < timestamps[1:][linked])).sum())
        assert hit >= 2
    # links between two segments: the last row of one and the first of the next, both inside, in one group
    step = batch.start_time[1:] - batch.end_time[:-1]
    joined = (corpus.run_groups[1:] == corpus.run_groups[:-1]) & (step > 0) & last_inside[:-1] & _in_spans(spans, batch.start_time[1:])
    assert int((joined & (step <= LINK_GAP)).sum()) >= 64 and int((joined & (step > LINK_GAP)).sum()) >= 8
    assert int((corpus.run_groups[1:] != corpus.run_groups[:-1]).sum()) >= 32   # (and neighbours that never link)


def episode_conditions(corpus):
    """The episodes of `band` under `run_groups` and EPISODE_GAP, from the oracle's grid alone: neighbours that both
    pass and are joined, neighbours that both pass and are cut by the gap rule, and passing rows in every group. (No two
    neighbours inside the band lie in different segments of these corpora: a run ends with its segment here, whatever
    the groups say.)"""
    batch = corpus.batch
    timestamps, values, lengths = ora.grid_batch(batch)[:3]
    timestamps = np.asarray(timestamps, dtype=np.int64)
    segment = np.repeat(np.arange(len(batch)), lengths.astype(np.int64))
    keys = _keys(values)
    passes = (keys >= int(_keys(np.float32(130.0)))) & (keys < int(_keys(np.float32(160.0))))
    both = passes[1:] & passes[:-1]
    group = corpus.run_groups.astype(np.int64)[segment]
    same_group = group[1:] == group[:-1]
    step = np.diff(timestamps)
    assert int((both & same_group & (step <= EPISODE_GAP)).sum()) >= 64
    assert int((both & same_group & (step > EPISODE_GAP)).sum()) >= 64
    assert all(int((passes & (group == g)).sum()) >= 64 for g in range(N_GROUPS))


def corpus_conditions(corpus, non_finite=True):
    """What the resident-state tests rely on a corpus to hold: conditions, not measurements."""
    partner_conditions(corpus)
    span_conditions(corpus, non_finite)
    episode_conditions(corpus)
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


# ---- the later operators --------------------------------------------------------------------------------------------
# CALLS[name](context, resident, corpus) makes the call and returns what it returned; MEMBERS[name](result) splits
# that into (exact, rounded): the members with ONE answer in the oracle - integers, timestamps, f32 values that are
# picked and not computed - and the f64 sums and moments, which two valid decoders may round differently. The digest
# of such an operator is digest(exact) + digest(rounded): compared as a whole everywhere, and `exact_part` of it where
# only the first half has to be the same (under another switch setting).

DIGEST_BYTES = hashlib.sha256().digest_size


def split_digest(exact, rounded):
    return digest(*exact) + digest(*rounded)


def exact_part(whole):
    assert len(whole) == 2 * DIGEST_BYTES
    return whole[:DIGEST_BYTES]


def upload(context, corpus):
    """The corpus's batch on the device and its partner's next to it, as `resident.partner`: for the life of a walk."""
    resident = context.upload_segments(corpus.batch)
    attach_partner(context, resident, corpus)
    return resident


def attach_partner(context, resident, corpus):
    resident.partner = context.upload_segments(corpus.partner.batch)


def release(resident):
    partner = getattr(resident, "partner", None)
    resident.free()
    if partner is not None:
        partner.free()


def _fields(names):
    def members(cells):
        return [np.ascontiguousarray(cells[name]) for name in names]
    return members


def _cells(exact, rounded):
    """MEMBERS of a structured array, or of a list of them: `exact` and `rounded` name every member."""
    exact_of, rounded_of = _fields(exact), _fields(rounded)

    def members(result):
        arrays = result if isinstance(result, (list, tuple)) else [result]
        for cells in arrays:
            assert set(cells.dtype.names) == set(exact) | set(rounded)
        return [exact_of(cells) for cells in arrays], [rounded_of(cells) for cells in arrays]
    return members


def _all_exact(result):
    return [result], []


def _bucket_request(corpus):
    origin, width, n_buckets = corpus.buckets
    return dict(origin=origin, width=width, n_buckets=n_buckets, t_lo=corpus.cut_range[0], t_hi=corpus.cut_range[1],
                n_groups=N_GROUPS)


def _call_m4(context, resident, corpus):
    return context.m4_buckets_dev(resident, groups=corpus.groups, **_bucket_request(corpus))


def _call_moments(context, resident, corpus):
    return context.moments_buckets_dev(resident, groups=corpus.groups, **_bucket_request(corpus))


def _call_hist_buckets(context, resident, corpus):
    return context.hist_buckets_dev(resident, corpus.edges, groups=corpus.groups, **_bucket_request(corpus))


def _call_quantile_buckets(context, resident, corpus):
    return context.quantile_buckets_dev(resident, QUANTILES, groups=corpus.groups, **_bucket_request(corpus))


def _call_comoments(context, resident, corpus):
    # x = the batch, y = its partner
    return context.comoments_buckets_dev(resident, resident.partner, groups=corpus.groups, **_bucket_request(corpus))


def _call_binned(context, resident, corpus):
    # x = the partner, y = the batch: the groups and the edges are x's
    partner = corpus.partner
    return context.binned_buckets_dev(resident.partner, resident, partner.edges, groups=partner.groups,
                                      **_bucket_request(corpus))


def _call_trend(context, resident, corpus):
    return context.trend_buckets_dev(resident, groups=corpus.groups, **_bucket_request(corpus))


def _over(spans):
    """One call per span of the corpus, in front of the gaps and behind: both answers."""
    def over(call):
        def run(context, resident, corpus):
            return [call(context, resident, corpus, origin, width, n) for origin, width, n in getattr(corpus, spans)]
        return run
    return over


@_over("spans")
def _call_integral(context, resident, corpus, origin, width, n_buckets):
    return context.integral_buckets_dev(resident, origin, width, n_buckets, groups=corpus.run_groups,
                                        method=mdb.MDB_INTEGRAL_LINEAR, max_gap=LINK_GAP, n_groups=N_GROUPS)


@_over("sample_spans")
def _call_sample(context, resident, corpus, origin, width, n_instants):
    return context.sample_at_dev(resident, origin, width, n_instants, groups=corpus.run_groups,
                                 method=mdb.MDB_SAMPLE_LINEAR, max_gap=LINK_GAP, n_groups=N_GROUPS)


@_over("sample_spans")
def _call_sample_step(context, resident, corpus, origin, width, n_instants):
    # (no gap rule: a value is carried over the 700 between two series too)
    return context.sample_at_dev(resident, origin, width, n_instants, groups=corpus.run_groups,
                                 method=mdb.MDB_SAMPLE_STEP, max_gap=None, n_groups=N_GROUPS)


@_over("spans")
def _call_change(context, resident, corpus, origin, width, n_buckets):
    return context.change_buckets_dev(resident, origin, width, n_buckets, groups=corpus.run_groups, max_gap=LINK_GAP,
                                      n_groups=N_GROUPS)


def _call_episodes(context, resident, corpus):
    return context.episodes_dev(resident, corpus.band, groups=corpus.run_groups, n_groups=N_GROUPS, max_gap=EPISODE_GAP)


EPISODE_EXACT = ("first_row", "count", "t_first", "t_last", "min", "max", "group", "first_segment", "reserved")


def _episode_members(result):
    episodes, n_rows, n_passing = result
    assert set(episodes.dtype.names) == set(EPISODE_EXACT) | {"sum"}
    return [_fields(EPISODE_EXACT)(episodes), n_rows, n_passing], [np.ascontiguousarray(episodes["sum"])]


COMOMENTS_ROUNDED = ("mean_x", "mean_y", "m2_x", "m2_y", "c_xy")
LATER = [
    ("m4", _call_m4, _all_exact),
    ("moments", _call_moments, _cells(("count",), ("mean", "m2"))),
    ("hist buckets", _call_hist_buckets, _all_exact),
    ("quantile buckets", _call_quantile_buckets, lambda result: (list(result), [])),
    ("comoments", _call_comoments, _cells(("count",), COMOMENTS_ROUNDED)),
    ("binned", _call_binned, _cells(("count",), ("mean", "m2"))),
    ("trend", _call_trend, _cells(("count",), COMOMENTS_ROUNDED)),
    ("integral", _call_integral, _cells(("duration",), ("integral",))),
    ("sample", _call_sample, _cells(("count",), ("sum",))),
    ("sample step", _call_sample_step, _cells(("count",), ("sum",))),
    ("change", _call_change, _cells(("count", "n_fall", "duration", "max_rise", "max_fall"), ("rise", "fall", "reset_sum"))),
    ("episodes", _call_episodes, _episode_members),
]
CALLS = {name: call for name, call, _ in LATER}
MEMBERS = {name: members for name, _, members in LATER}


def _later(name):
    def run(context, resident, corpus):
        return split_digest(*MEMBERS[name](CALLS[name](context, resident, corpus)))
    return run


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
] + [(name, _later(name)) for name, _, _ in LATER]
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

def _extra_row(corpus):
    """A MacaqueV segment of the corpus of a few hundred values, moved behind its last segment."""
    batch = corpus.batch
    lengths = layouts.macaque_v_lengths(batch)
    rows = np.flatnonzero(batch.model_type_id == mdb.MDB_MACAQUE_V_ID)
    residuals = batch.residuals.to_bytes_list()
    picked = [int(r) for r, n in zip(rows, lengths) if 200 <= n <= 400 and not residuals[r]]
    assert picked
    row = list(batch.rows()[picked[0]])
    shift = int(batch.end_time[-1]) + 700 - row[1]   # (behind the last segment: the series stays ascending)
    row[1], row[2] = row[1] + shift, row[2] + shift
    return row


def malformed(corpus):
    """The corpus plus ONE row: a MacaqueV segment of a few hundred values whose `values` payload is cut to half its
    bytes, everything else as it was (the count the timestamps claim too)."""
    row = _extra_row(corpus)
    row[6] = row[6][: len(row[6]) // 2]
    return mdb.SegmentBatch.concat([corpus.batch, mdb.SegmentBatch.from_rows([tuple(row)])])


def malformed_corpus(corpus):
    """`malformed(corpus)` with what is asked about the corpus, and as its partner the corpus's partner plus the same
    extra row with its payload whole: the pair lines up, and its only fault is the one cut stream."""
    row = _extra_row(corpus)
    other = corpus.partner
    whole = mdb.SegmentBatch.concat([other.batch, mdb.SegmentBatch.from_rows([tuple(row)])])
    partner = Corpus("malformed's partner", whole, other.timestamps, other.values)
    return Corpus("malformed", malformed(corpus), corpus.timestamps, corpus.values, partner=partner)
