"""The tables and the oracle of tests/test_gpu_comoments.py: several series, every field compressed on its own by
ora.try_compress_univariate_time_series under its own error bound (as tests/test_gpu_row_mask.py builds its tables), so
the same series is cut into different segments per field; and the cells of a pair of fields computed from the oracle's
grids in exact arithmetic (math.fsum)."""

import math

import numpy as np

import cases
import datagen
import oracle_lib as ora
import modelardb_rs_amd as mdb

INTERVAL = 100  # the sampling interval of tests/datagen.py
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MEAN_TOLERANCE = 2.0 ** -44   # of the largest |v| of the cell and field
M2_TOLERANCE = 1e-5           # of m2_ref
C_TOLERANCE = 1e-5            # of sqrt(m2x_ref * m2y_ref), the Cauchy-Schwarz bound of |c|
MEMBERS = ("mean_x", "mean_y", "m2_x", "m2_y", "c_xy")


class Field:
    """One field column of a table: its segments (all series, in series order), the series of every segment and the
    oracle's grid of them."""

    def __init__(self, parts):
        self.parts = list(parts)   # one batch per series
        self.batch = mdb.SegmentBatch.concat(self.parts)
        self.groups = np.concatenate([np.full(len(part), k, dtype=np.uint32) for k, part in enumerate(self.parts)])
        ts, values, rows, _ = ora.grid_batch(self.batch)
        self.ts, self.values, self.rows = ts.astype(np.int64), values.astype(np.float32), rows.astype(np.int64)
        self.segment = np.repeat(np.arange(len(self.batch)), self.rows)
        self.dev = None

    def in_range(self, t_lo, t_hi):
        return (self.ts >= t_lo) & (self.ts <= t_hi)

    def resident(self, context):
        if self.dev is None:
            self.dev = context.upload_segments(self.batch)
        return self.dev

    def free(self):
        if self.dev is not None:
            self.dev.free()
            self.dev = None


def table(series, bounds):
    """series: [(timestamps, [values of field 0, values of field 1, ...])]; bounds: one error bound per field."""
    return [Field([ora.try_compress_univariate_time_series(ts, values[f], eb) for ts, values in series])
            for f, eb in enumerate(bounds)]


def _series(length, irregular, seeds, segment_length_range=(50, 501), t0=0):
    timestamps, values = None, []
    for seed in seeds:
        ts, v = datagen.generate_univariate_time_series(length, segment_length_range, irregular, (1.0, 1.05),
                                                        (100.0, 200.0), seed)
        timestamps = ts if timestamps is None else timestamps
        values.append(v)
    return timestamps + t0, values


_TABLES = {}


def main_table():
    """Three fields (lossless, 1 % relative, absolute 5) of four series: regular and irregular timestamps, a sine with
    segments far longer than 64 rows, runs of 2..12 points with segments far shorter."""
    if "main" not in _TABLES:
        sine_ts = 5_000 + np.arange(12_000, dtype=np.int64) * INTERVAL
        sines = [datagen.sine_series(k, 12_000)[1] for k in (3, 4, 5)]
        series = [_series(6000, False, (11, 12, 13)), _series(5000, True, (21, 22, 23), t0=30_000),
                  (sine_ts, sines), _series(1500, False, (31, 32, 33), segment_length_range=(2, 12), t0=700_000)]
        bounds = cases.error_bounds()
        _TABLES["main"] = table(series, [bounds["lossless"], bounds["rel1"], bounds["abs5"]])
    return _TABLES["main"]


def edge_table():
    """The series of cases.edge_case_batch() (NaN, +-0, +-inf, epoch-scale Swing) and their partner: the same series
    under absolute 5. Each series a group."""
    if "edge" not in _TABLES:
        _TABLES["edge"] = [Field([ora.try_compress_univariate_time_series(ts, v, eb) for _, ts, v in cases.edge_case_series()])
                           for eb in (cases.LOSSLESS, cases.error_bounds()["abs5"])]
        assert _TABLES["edge"][0].batch.identical(cases.edge_case_batch())
    return _TABLES["edge"]


def steps_table():
    """Two fields of one series, lossless: levels held for 500 points each (PMC-Mean runs) and noise."""
    if "steps" not in _TABLES:
        rng = np.random.default_rng(77)
        n = 6_000
        timestamps = np.arange(n, dtype=np.int64) * INTERVAL
        levels = np.repeat(rng.normal(50.0, 20.0, n // 500).astype(np.float32), 500)
        noisy = (100.0 + rng.normal(0.0, 3.0, n)).astype(np.float32)
        _TABLES["steps"] = table([(timestamps, [levels, noisy])], [cases.LOSSLESS, cases.LOSSLESS])
    return _TABLES["steps"]


def free_tables():
    for fields in _TABLES.values():
        for field in fields:
            field.free()


def assert_lined_up(fields, ranges):
    """The precondition of the data: the oracle alone gives the same rows (count and timestamps) for every field."""
    for t_lo, t_hi in ranges:
        picked = [field.ts[field.in_range(t_lo, t_hi)] for field in fields]
        for other in picked[1:]:
            assert len(other) == len(picked[0]) and np.array_equal(other, picked[0]), (t_lo, t_hi)


def bucket_sets(first, last):
    """(name, origin, width, n_buckets, t_lo, t_hi) over data in [first, last]: those of tests/test_gpu_moments.py."""
    span = last - first + 1
    return [
        ("width_1_interval", first, INTERVAL, span // INTERVAL + 1, I64_MIN, I64_MAX),
        ("width_7_intervals", first, 7 * INTERVAL, span // (7 * INTERVAL) + 1, I64_MIN, I64_MAX),
        ("width_1000_intervals", first, 1000 * INTERVAL, span // (1000 * INTERVAL) + 1, I64_MIN, I64_MAX),
        ("one_bucket", first, span, 1, I64_MIN, I64_MAX),
        ("unaligned_origin_before", first - 12_345, 3_333, (span + 12_345) // 3_333 + 2, I64_MIN, I64_MAX),
        ("buckets_after_the_data", last + 1, 1000, 50, I64_MIN, I64_MAX),
        ("range_cuts_buckets", first - 50, 5_000, span // 5_000 + 2, first + 7_777, last - 12_321),
    ]


def cell_reference(x, y):
    """(mean_x, mean_y, m2_x, m2_y, c) of the f32 pairs of one cell, in exact arithmetic."""
    dx = x.astype(np.float64) - float(x[0])
    dy = y.astype(np.float64) - float(y[0])
    n = len(dx)
    shift_x, shift_y = math.fsum(dx) / n, math.fsum(dy) / n
    rx, ry = dx - shift_x, dy - shift_y
    return float(x[0]) + shift_x, float(y[0]) + shift_y, math.fsum(rx * rx), math.fsum(ry * ry), math.fsum(rx * ry)


def _point_buckets(timestamps, origin, width):
    if len(timestamps) == 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = int(timestamps.min()) - origin, int(timestamps.max()) - origin
    if I64_MIN <= lo and hi <= I64_MAX:
        return (timestamps - np.int64(origin)) // np.int64(width)
    buckets = [(int(t) - origin) // width for t in timestamps]
    return np.array([b if 0 <= b <= I64_MAX else -1 for b in buckets], dtype=np.int64)


def oracle(x, y, groups, n_groups, origin, width, n_buckets, t_lo=I64_MIN, t_hi=I64_MAX):
    """The cells of the pair (x, y) from the oracle's grids: row r of x under [t_lo, t_hi] with row r of y, in the
    bucket of its x-side timestamp and the group of its x-side segment. Per cell the count, the five members in exact
    arithmetic, the largest |v| of either field and whether every point of either field is finite."""
    keep_x, keep_y = x.in_range(t_lo, t_hi), y.in_range(t_lo, t_hi)
    assert int(keep_x.sum()) == int(keep_y.sum())
    ts, xv, yv = x.ts[keep_x], x.values[keep_x], y.values[keep_y]
    groups = np.zeros(len(x.batch), dtype=np.uint32) if groups is None else groups
    point_groups = groups.astype(np.int64)[x.segment[keep_x]]
    buckets = _point_buckets(ts, origin, width)
    keep = (buckets >= 0) & (buckets < n_buckets)
    cells = point_groups[keep] * n_buckets + buckets[keep]
    xv, yv = xv[keep], yv[keep]
    n_cells = n_groups * n_buckets
    out = {"count": np.zeros(n_cells, dtype=np.int64), "largest_x": np.zeros(n_cells), "largest_y": np.zeros(n_cells),
           "finite_x": np.ones(n_cells, dtype=bool), "finite_y": np.ones(n_cells, dtype=bool)}
    out.update({name: np.zeros(n_cells) for name in MEMBERS})
    if len(cells):
        order = np.argsort(cells, kind="stable")
        sorted_cells, xs, ys = cells[order], xv[order], yv[order]
        starts = np.flatnonzero(np.concatenate([[True], sorted_cells[1:] != sorted_cells[:-1]]))
        ends = np.concatenate([starts[1:], [len(cells)]])
        with np.errstate(invalid="ignore", over="ignore"):
            for start, end in zip(starts, ends):
                cell, run_x, run_y = sorted_cells[start], xs[start:end], ys[start:end]
                out["count"][cell] = end - start
                out["finite_x"][cell] = bool(np.isfinite(run_x).all())
                out["finite_y"][cell] = bool(np.isfinite(run_y).all())
                if out["finite_x"][cell] and out["finite_y"][cell]:
                    reference = cell_reference(run_x, run_y)
                    for name, value in zip(MEMBERS, reference):
                        out[name][cell] = value
                    out["largest_x"][cell] = float(np.abs(run_x.astype(np.float64)).max())
                    out["largest_y"][cell] = float(np.abs(run_y.astype(np.float64)).max())
    return {name: array.reshape(n_groups, n_buckets) for name, array in out.items()}


def assert_cells(got, expected, context="", fresh=True):
    """count exact; in a cell of finite points each mean within 2^-44 of the cell's largest |v| of that field, each m2
    within 1e-5 of its reference, c_xy within 1e-5 of sqrt(m2x_ref * m2y_ref); in a cell with a non-finite point in a
    field that field's mean and m2 and c_xy are not finite. `fresh`: the call began with fresh cells, so a cell
    without pairs is all-zero bytes still. Prints the worst ratios."""
    assert got.shape == expected["count"].shape, context
    np.testing.assert_array_equal(got["count"], expected["count"], err_msg=context)
    hit = expected["count"] > 0
    if fresh:
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * mdb.COMOMENTS_CELL_DTYPE.itemsize), context
    for field in ("x", "y"):
        special = hit & ~expected["finite_" + field]
        for name in ("mean_" + field, "m2_" + field, "c_xy"):
            assert not np.isfinite(got[name][special]).any(), (context, name)
    plain = hit & expected["finite_x"] & expected["finite_y"]
    for name in MEMBERS:
        assert np.isfinite(got[name][plain]).all(), (context, name)
    worst, checks = {}, []
    with np.errstate(invalid="ignore", divide="ignore"):
        for field in ("x", "y"):
            mean_error = np.abs(got["mean_" + field][plain] - expected["mean_" + field][plain])
            m2_error = np.abs(got["m2_" + field][plain] - expected["m2_" + field][plain])
            worst["mean_" + field] = np.nan_to_num(mean_error / expected["largest_" + field][plain]).max(initial=0.0)
            worst["m2_" + field] = np.nan_to_num(m2_error / expected["m2_" + field][plain]).max(initial=0.0)
            checks.append((mean_error <= MEAN_TOLERANCE * expected["largest_" + field][plain], "mean_" + field))
            checks.append((m2_error <= M2_TOLERANCE * expected["m2_" + field][plain], "m2_" + field))  # (m2_ref == 0: 0.0)
            checks.append((got["m2_" + field][plain] >= 0.0, "m2_" + field + " >= 0"))
        scale = np.sqrt(expected["m2_x"][plain] * expected["m2_y"][plain])
        c_error = np.abs(got["c_xy"][plain] - expected["c_xy"][plain])
        worst["c_xy"] = np.nan_to_num(c_error / scale).max(initial=0.0)
        checks.append((c_error <= C_TOLERANCE * scale, "c_xy"))   # (either m2_ref == 0: c_xy == 0.0)
    print(f"{context}: {int(plain.sum())} cells, mean error / max|v| <= {max(worst['mean_x'], worst['mean_y']):.3g} "
          f"(allowed {MEAN_TOLERANCE:.3g}), m2 error / m2 <= {max(worst['m2_x'], worst['m2_y']):.3g} (allowed "
          f"{M2_TOLERANCE:.3g}), c error / sqrt(m2x m2y) <= {worst['c_xy']:.3g} (allowed {C_TOLERANCE:.3g})")
    for within, name in checks:
        assert within.all(), (context, name)
