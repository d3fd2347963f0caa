"""The oracle of tests/test_gpu_trend.py: the cells of mdb_trend_buckets* for one field of tests/comoments_cases.py's
tables, from the oracle's grid of the field (Field.ts / Field.values) with x = (t - origin) mod width - the time offset
of the point inside its bucket - and y = the value, per cell in exact arithmetic (comoments_cases.cell_reference,
math.fsum). Assertions are comoments_cases.assert_cells with its tolerances; nothing here calls the library under
test."""

import numpy as np

import comoments_cases as cc

I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
INTERVAL = cc.INTERVAL


def offsets(timestamps, origin, width):
    """(bucket, x) per timestamp: bucket = floor((t - origin) / width) (-1: below bucket 0 or beyond int64) and
    x = (t - origin) - bucket * width as f64, from integers (exact below 2^53)."""
    buckets = cc._point_buckets(timestamps, origin, width)
    if len(timestamps) == 0:
        return buckets, np.zeros(0, dtype=np.float64)
    if I64_MIN <= int(timestamps.min()) - origin and int(timestamps.max()) - origin <= I64_MAX:
        return buckets, ((timestamps - np.int64(origin)) - buckets * np.int64(width)).astype(np.float64)
    x = [float((int(t) - origin) - int(b) * width) if b >= 0 else 0.0 for t, b in zip(timestamps, buckets)]
    return buckets, np.array(x, dtype=np.float64)


def oracle(field, groups, n_groups, origin, width, n_buckets, t_lo=I64_MIN, t_hi=I64_MAX):
    """The cells of `field` (a comoments_cases.Field) in the shape comoments_cases.assert_cells takes: the count, the
    five members in exact arithmetic where every value of the cell is finite, the largest |x| and |v|, finite_x (always)
    and finite_y. Beside them x_mean and x_m2: the x side of EVERY cell with points, finite values or not."""
    keep = field.in_range(t_lo, t_hi)
    ts, values = field.ts[keep], field.values[keep]
    groups = np.zeros(len(field.batch), dtype=np.uint32) if groups is None else groups
    point_groups = groups.astype(np.int64)[field.segment[keep]]
    buckets, x = offsets(ts, origin, width)
    inside = (buckets >= 0) & (buckets < n_buckets)
    cells = point_groups[inside] * n_buckets + buckets[inside]
    x, values = x[inside], values[inside]
    n_cells = n_groups * n_buckets
    out = {"count": np.zeros(n_cells, dtype=np.int64), "largest_x": np.zeros(n_cells), "largest_y": np.zeros(n_cells),
           "finite_x": np.ones(n_cells, dtype=bool), "finite_y": np.ones(n_cells, dtype=bool),
           "x_mean": np.zeros(n_cells), "x_m2": np.zeros(n_cells)}
    out.update({name: np.zeros(n_cells) for name in cc.MEMBERS})
    if len(cells):
        order = np.argsort(cells, kind="stable")
        sorted_cells, xs, ys = cells[order], x[order], values[order]
        starts = np.flatnonzero(np.concatenate([[True], sorted_cells[1:] != sorted_cells[:-1]]))
        ends = np.concatenate([starts[1:], [len(cells)]])
        with np.errstate(invalid="ignore", over="ignore"):
            for start, end in zip(starts, ends):
                cell, run_x, run_y = sorted_cells[start], xs[start:end], ys[start:end]
                out["count"][cell] = end - start
                out["finite_y"][cell] = bool(np.isfinite(run_y).all())
                out["largest_x"][cell] = float(np.abs(run_x).max())
                if out["finite_y"][cell]:
                    reference = cc.cell_reference(run_x, run_y)
                    for name, value in zip(cc.MEMBERS, reference):
                        out[name][cell] = value
                    out["largest_y"][cell] = float(np.abs(run_y.astype(np.float64)).max())
                else:
                    reference = cc.cell_reference(run_x, np.zeros(len(run_x), dtype=np.float32))
                out["x_mean"][cell], out["x_m2"][cell] = reference[0], reference[2]
    return {name: array.reshape(n_groups, n_buckets) for name, array in out.items()}


def assert_x_side(got, expected, context=""):
    """mean_x and m2_x of every cell with points - those whose values are not finite too - finite and within
    comoments_cases' tolerances of the reference. Returns how many of the cells hold a non-finite value."""
    hit = expected["count"] > 0
    assert np.isfinite(got["mean_x"][hit]).all() and np.isfinite(got["m2_x"][hit]).all(), context
    assert (np.abs(got["mean_x"][hit] - expected["x_mean"][hit]) <= cc.MEAN_TOLERANCE * expected["largest_x"][hit]).all(), context
    assert (np.abs(got["m2_x"][hit] - expected["x_m2"][hit]) <= cc.M2_TOLERANCE * expected["x_m2"][hit]).all(), context
    return int((hit & ~expected["finite_y"]).sum())
