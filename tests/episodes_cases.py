"""TEST INFRASTRUCTURE: the cases and the reference of the episode tests (tests/test_gpu_episodes.py).

The reference is the oracle's grid of a batch plus numpy: the totalOrder keys of the values as
tests/test_gpu_value_filter.py builds them, the "continues" rule on the row arrays, np.fmin / np.fmax from the FLT_MAX
initials and math.fsum for the sum. Nothing here calls the library under test."""

import math

import numpy as np

import cases
import datagen
import oracle_lib as ora
import modelardb_rs_amd as mdb

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
F32_MAX = np.float32(np.finfo(np.float32).max)
SUM_TOLERANCE = 1e-5  # of the sum of magnitudes: the tolerance of the filtered aggregates
EXACT_FIELDS = ("first_row", "count", "t_first", "t_last", "group", "first_segment", "reserved")


class Table:
    """A batch and the oracle's grid of it: timestamps, values and the segment row of every grid row."""

    def __init__(self, batch):
        self.batch = batch
        self.ts, self.values, self.rows, _ = ora.grid_batch(batch)
        self.segment = np.repeat(np.arange(len(batch)), self.rows.astype(np.int64))
        self.dev = None


def keys_of(values):
    bits = np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def key_bounds(flt):
    lo_bits, hi_bits = mdb.value_filter_bits(flt)
    lo = -(1 << 31) if flt.flags & 4 else int(keys_of(np.uint32(lo_bits).view(np.float32))) + (1 if flt.flags & 1 else 0)
    hi = (1 << 31) - 1 if flt.flags & 8 else int(keys_of(np.uint32(hi_bits).view(np.float32))) - (1 if flt.flags & 2 else 0)
    return lo, hi


def reference(table, flt, groups=None, max_gap=None, min_duration=0, min_count=0):
    """(episodes of mdb.EPISODE_DTYPE, sum of magnitudes per episode, n_rows, n_passing, pass bits)."""
    inside = (table.ts >= flt.t_lo) & (table.ts <= flt.t_hi)
    ts, values, segment = table.ts[inside], table.values[inside], table.segment[inside]
    n = len(ts)
    group_of_segment = np.zeros(len(table.batch), dtype=np.uint32) if groups is None else np.asarray(groups, dtype=np.uint32)
    group = group_of_segment[segment] if n else np.zeros(0, dtype=np.uint32)
    lo, hi = key_bounds(flt)
    keys = keys_of(values)
    passes = (keys >= lo) & (keys <= hi)
    max_gap = I64_MAX if max_gap is None else int(max_gap)
    continues = np.zeros(n, dtype=bool)
    if n > 1:
        forward = ts[1:] >= ts[:-1]
        # (formed as uint64 after the comparison: where forward holds the wrapped difference is the true one)
        step = ts[1:].view(np.uint64) - ts[:-1].view(np.uint64)
        continues[1:] = (group[1:] == group[:-1]) & forward & (step <= np.uint64(max_gap))
    before = np.concatenate([[False], passes[:-1]]) if n else passes
    starts = np.flatnonzero(passes & ~(before & continues))
    after_joins = np.concatenate([passes[1:] & continues[1:], [False]]) if n else passes
    ends = np.flatnonzero(passes & ~after_joins)
    assert len(starts) == len(ends) and np.all(starts <= ends)
    out = np.zeros(len(starts), dtype=mdb.EPISODE_DTYPE)
    magnitudes = np.zeros(len(starts))
    wide = values.astype(np.float64)
    for k, (a, b) in enumerate(zip(starts.tolist(), ends.tolist())):
        run, run_wide = values[a:b + 1], wide[a:b + 1]
        with np.errstate(invalid="ignore"):  # (inf - inf is the NaN the sum must be)
            total = math.fsum(run_wide) if np.all(np.isfinite(run_wide)) else float(np.sum(run_wide))
        out[k] = (a, b - a + 1, ts[a], ts[b], total, np.fmin.reduce(np.concatenate([[F32_MAX], run])),
                  np.fmax.reduce(np.concatenate([[-F32_MAX], run])), group[a], segment[a], 0)
        magnitudes[k] = math.fsum(np.abs(run_wide[np.isfinite(run_wide)]))
    duration = out["t_last"].astype(object) - out["t_first"].astype(object) if len(out) else np.zeros(0, dtype=object)
    kept = np.array([int(c) >= int(min_count) and int(d) >= int(min_duration) for c, d in zip(out["count"], duration)],
                    dtype=bool) if len(out) else np.zeros(0, dtype=bool)
    return out[kept], magnitudes[kept], n, int(passes.sum()), passes


def assert_episodes(got, expected, magnitudes):
    """Every field exact but `sum` (within SUM_TOLERANCE of the sum of magnitudes, NaN where the reference's is).
    min and max are compared as numbers: fmin / fmax leave the sign of a zero extreme open."""
    assert got.dtype == mdb.EPISODE_DTYPE
    assert len(got) == len(expected), (len(got), len(expected))
    for field in EXACT_FIELDS:
        assert np.array_equal(got[field], expected[field]), field
    for field in ("min", "max"):
        assert not np.isnan(got[field]).any() and np.array_equal(got[field], expected[field]), field
    nan = np.isnan(expected["sum"])
    assert np.array_equal(np.isnan(got["sum"]), nan)
    infinite = np.isinf(expected["sum"])
    assert np.array_equal(got["sum"][infinite], expected["sum"][infinite])
    finite = ~nan & ~infinite
    error = np.abs(got["sum"][finite] - expected["sum"][finite])
    assert np.all(error <= SUM_TOLERANCE * magnitudes[finite]), float(np.max(error - SUM_TOLERANCE * magnitudes[finite]))


def same_but_sum(a, b):
    """Byte equality of two episode arrays apart from `sum`."""
    if len(a) != len(b):
        return False
    a, b = a.copy(), b.copy()
    a["sum"] = 0.0
    b["sum"] = 0.0
    return a.tobytes() == b.tobytes()


# ---- tables -------------------------------------------------------------------------------------------------------

def main_series():
    """Four series of 1 500 - 12 000 points: regular and irregular timestamps, a sine with segments far longer than
    64 rows, runs of 2..12 points with segments far shorter."""
    def one(length, irregular, seed, lengths=(50, 501), t0=0):
        ts, v = datagen.generate_univariate_time_series(length, lengths, irregular, (1.0, 1.05), (100.0, 200.0), seed)
        return ts + t0, v
    sine_ts = 5_000 + np.arange(12_000, dtype=np.int64) * 100
    return [one(6000, False, 11), one(5000, True, 21, t0=30_000), (sine_ts, datagen.sine_series(3, 12_000)[1]),
            one(1500, False, 31, lengths=(2, 12), t0=700_000)]


_TABLES = {}


def main_tables():
    """The main series under lossless, 1 % relative and absolute 5: PMC-Mean, Swing, MacaqueV and residual tails all
    occur. One table per error bound; group_of_segment = the series of the segment."""
    if "main" not in _TABLES:
        bounds = cases.error_bounds()
        tables = []
        for name in ("lossless", "rel1", "abs5"):
            parts = [ora.try_compress_univariate_time_series(ts, v, bounds[name]) for ts, v in main_series()]
            table = Table(mdb.SegmentBatch.concat(parts))
            table.groups = np.repeat(np.arange(len(parts), dtype=np.uint32), [len(p) for p in parts])
            tables.append(table)
        _TABLES["main"] = tables
    return _TABLES["main"]


def edge_table():
    if "edge" not in _TABLES:
        _TABLES["edge"] = Table(cases.edge_case_batch())
    return _TABLES["edge"]


EDGE_EPOCH = 1658671178037


def time_ranges(table):
    """The whole axis, a range that clips segments mid-way, a range that matches nothing."""
    first, last = int(table.ts.min()), int(table.ts.max())
    if table is _TABLES.get("edge"):
        return [(I64_MIN, I64_MAX), (150, 950), (EDGE_EPOCH + 100_500, EDGE_EPOCH + 300_400), (last + 10, last + 1000)]
    return [(I64_MIN, I64_MAX), (first + (last - first) // 5 + 37, last - (last - first) // 3 - 11), (last + 10, last + 1000)]


def predicates(table):
    """(name, value_filter keyword arguments): always true, always false, an empty interval, thresholds at stored
    values and their float neighbours, open and closed, and a band [lo, hi)."""
    finite = table.values[np.isfinite(table.values)]
    median = np.float32(np.median(finite))
    stored = np.float32(finite[len(finite) // 3])
    out = [("all", {}), ("none", {"lo": 1e39}), ("empty", {"lo": 5.0, "hi": 1.0}),
           ("gt_median", {"lo": float(median), "lo_open": True}), ("le_median", {"hi": float(median)})]
    for name, value in (("stored", stored), ("above", np.nextafter(stored, np.float32(np.inf))),
                        ("below", np.nextafter(stored, np.float32(-np.inf)))):
        out.append((f"ge_{name}", {"lo": float(value)}))
        out.append((f"lt_{name}", {"hi": float(value), "hi_open": True}))
    out.append(("gt_stored", {"lo": float(stored), "lo_open": True}))
    out.append(("le_stored", {"hi": float(stored)}))
    low, high = np.float32(np.quantile(finite, 0.3)), np.float32(np.quantile(finite, 0.7))
    out.append(("band", {"lo": float(low), "hi": float(high), "hi_open": True}))
    return out


def pmc_rows(starts_values_counts, delta=100):
    """Hand-built PMC-Mean segments on regular timestamps: (start, value, n_points) each."""
    rows = []
    for start, value, n in starts_values_counts:
        stream = b"" if n <= 2 else int(n).to_bytes(1 if n < 128 else 2 if n < 32768 else 4, "big")
        rows.append((mdb.MDB_PMC_MEAN_ID, int(start), int(start + (n - 1) * delta), stream, float(value), float(value), b"", b""))
    return rows
