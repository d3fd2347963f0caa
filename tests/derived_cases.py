"""The cases and the reference of the derived-field tests (tests/test_derived_cpu.py, tests/test_gpu_derived.py,
tests/test_gpu_derived_soak.py): z = f(x, y) by numpy float32 in the written order on the oracle's grids of x and y
under the time range, and per cell the count, min and max (the rule of mdb_agg_buckets' MIN and MAX) and mean / m2 by
math.fsum around the first value, as tests/test_comoments_cpu.py::_reference does. Fields are
comoments_cases.Field (or anything with its batch, ts, values, segment and in_range)."""

import math

import numpy as np

import comoments_cases as cc
import modelardb_rs_amd as mdb

INTERVAL = cc.INTERVAL
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
MEAN_TOLERANCE = 2.0 ** -44   # of the largest |z| of the cell (mdb.h, tests/test_comoments_cpu.py)
M2_TOLERANCE = 1e-5           # of m2_ref
FLT_MAX = np.float32(3.4028234663852886e38)
SHORT, CHUNK = mdb.MDB_DERIVED_SHORT_ROWS, mdb.MDB_DERIVED_CHUNK_ROWS

# (op, a, b, c, absolute): every op with and without ABS; coefficients 1, -1, 0 and an inexact one
EXPRESSIONS = {
    "difference": ("linear", 1.0, -1.0, 0.0, False),
    "absolute_difference": ("linear", 1.0, -1.0, 0.0, True),
    "weighted_sum": ("linear", 0.1, 1.7, -3.3, False),
    "x_alone": ("linear", 1.0, 0.0, 0.0, False),
    "product": ("product", 1.0, 0.0, 0.0, False),
    "scaled_product": ("product", -0.3, 0.0, 2.5, True),
    "ratio": ("ratio", 1.0, 0.0, 0.0, False),
    "scaled_ratio": ("ratio", 0.7, 0.0, -1.0, True),
}


def expression(name_or_tuple):
    op, a, b, c, absolute = EXPRESSIONS[name_or_tuple] if isinstance(name_or_tuple, str) else name_or_tuple
    return mdb.derived_expr(op, a, b, c, absolute)


def z_of(expr, x, y):
    """numpy float32, one rounding per operation, in the written order."""
    op, a, b, c, absolute = EXPRESSIONS[expr] if isinstance(expr, str) else expr
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    with np.errstate(all="ignore"):
        if op == "linear":
            z = ((a * x) + (b * y)) + c
        elif op == "product":
            z = (a * (x * y)) + c
        else:
            z = (a * (x / y)) + c
        z = z.astype(np.float32)
    if absolute:
        z = (z.view(np.uint32) & np.uint32(0x7FFFFFFF)).view(np.float32)
    return z


def column(x, y, expr, t_lo=I64_MIN, t_hi=I64_MAX):
    """(timestamps of x, z) of the rows under [t_lo, t_hi]."""
    keep_x, keep_y = x.in_range(t_lo, t_hi), y.in_range(t_lo, t_hi)
    assert int(keep_x.sum()) == int(keep_y.sum())
    return x.ts[keep_x], z_of(expr, x.values[keep_x], y.values[keep_y])


def cell_reference(z):
    """(mean, m2, min, max) of the f32 values of one cell: mean and m2 in exact arithmetic around the first value; min
    and max by the aggregates' rule (from FLT_MAX / -FLT_MAX, NaNs skipped)."""
    numbers = z[~np.isnan(z)]
    low = min(FLT_MAX, numbers.min()) if len(numbers) else FLT_MAX
    high = max(-FLT_MAX, numbers.max()) if len(numbers) else -FLT_MAX
    if not np.isfinite(z).all():   # (neither mean nor m2 is finite then, and nothing more is promised)
        return math.nan, math.nan, np.float32(low), np.float32(high)
    d = z.astype(np.float64) - float(z[0])
    shift = math.fsum(d) / len(d)
    r = d - shift
    return float(z[0]) + shift, math.fsum(r * r), np.float32(low), np.float32(high)


def oracle(x, y, expr, groups, n_groups, origin, width, n_buckets, t_lo=I64_MIN, t_hi=I64_MAX):
    keep_x = x.in_range(t_lo, t_hi)
    ts, z = column(x, y, expr, t_lo, t_hi)
    groups = np.zeros(len(x.batch), dtype=np.uint32) if groups is None else groups
    point_groups = groups.astype(np.int64)[x.segment[keep_x]]
    buckets = cc._point_buckets(ts, origin, width)
    keep = (buckets >= 0) & (buckets < n_buckets)
    cells = point_groups[keep] * n_buckets + buckets[keep]
    z = z[keep]
    n_cells = n_groups * n_buckets
    out = {"count": np.zeros(n_cells, dtype=np.int64), "mean": np.zeros(n_cells), "m2": np.zeros(n_cells),
           "min": np.zeros(n_cells, dtype=np.float32), "max": np.zeros(n_cells, dtype=np.float32),
           "largest": np.zeros(n_cells), "finite": np.ones(n_cells, dtype=bool)}
    if len(cells):
        order = np.argsort(cells, kind="stable")
        sorted_cells, zs = cells[order], z[order]
        starts = np.flatnonzero(np.concatenate([[True], sorted_cells[1:] != sorted_cells[:-1]]))
        ends = np.concatenate([starts[1:], [len(cells)]])
        with np.errstate(invalid="ignore", over="ignore"):
            for start, end in zip(starts, ends):
                cell, run = sorted_cells[start], zs[start:end]
                out["count"][cell] = end - start
                out["finite"][cell] = bool(np.isfinite(run).all())
                mean, m2, low, high = cell_reference(run)
                out["min"][cell], out["max"][cell] = low, high
                if out["finite"][cell]:
                    out["mean"][cell], out["m2"][cell] = mean, m2
                    out["largest"][cell] = float(np.abs(run.astype(np.float64)).max())
    return {name: array.reshape(n_groups, n_buckets) for name, array in out.items()}


def assert_exact_members(got, expected, context="", fresh=True):
    """count, min and max: exact (min and max compared with ==: -0.0 and +0.0 are one extreme, mdb.h)."""
    assert got.shape == expected["count"].shape, context
    np.testing.assert_array_equal(got["count"], expected["count"], err_msg=str(context))
    hit = expected["count"] > 0
    if fresh:
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * mdb.DERIVED_CELL_DTYPE.itemsize), context
    np.testing.assert_array_equal(got["min"][hit], expected["min"][hit], err_msg=f"{context} min")
    np.testing.assert_array_equal(got["max"][hit], expected["max"][hit], err_msg=f"{context} max")


def assert_cells(got, expected, context="", fresh=True):
    """count, min, max exact; in a cell of finite z the mean within 2^-44 of the largest |z| and m2 within 1e-5 of its
    reference; in a cell with a non-finite z neither mean nor m2 is finite. Prints the worst ratios."""
    assert_exact_members(got, expected, context, fresh)
    hit = expected["count"] > 0
    special = hit & ~expected["finite"]
    assert not np.isfinite(got["mean"][special]).any() and not np.isfinite(got["m2"][special]).any(), context
    plain = hit & expected["finite"]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_error = np.abs(got["mean"][plain] - expected["mean"][plain])
        m2_error = np.abs(got["m2"][plain] - expected["m2"][plain])
        worst_mean = np.nan_to_num(mean_error / expected["largest"][plain]).max(initial=0.0)
        worst_m2 = np.nan_to_num(m2_error / expected["m2"][plain]).max(initial=0.0)
    print(f"{context}: {int(plain.sum())} cells, mean error / max|z| <= {worst_mean:.3g} (allowed {MEAN_TOLERANCE:.3g}), "
          f"m2 error / m2 <= {worst_m2:.3g} (allowed {M2_TOLERANCE:.3g})")
    assert (mean_error <= MEAN_TOLERANCE * expected["largest"][plain]).all(), (context, "mean", worst_mean)
    assert (m2_error <= M2_TOLERANCE * expected["m2"][plain]).all(), (context, "m2", worst_m2)   # (m2_ref == 0: 0.0)
    assert (got["m2"][plain] >= 0.0).all(), (context, "m2 >= 0")


def cells_of(runs):
    """The exact cells of runs of z values (empty runs: fresh cells)."""
    cells = mdb.fresh_derived_cells(len(runs))
    for k, run in enumerate(runs):
        if len(run):
            mean, m2, low, high = cell_reference(run)
            cells[k] = (len(run), mean, m2, low, high)
    return cells


def data_sets(rng, n):
    """The project's data sets: levels 0, 1e6 and 1e7 with sigma 0.5 - (x, y) pairs of float32."""
    return {f"level_{level:g}": ((level + rng.normal(0.0, 0.5, n)).astype(np.float32),
                                 (level + rng.normal(0.0, 0.5, n)).astype(np.float32)) for level in (0.0, 1.0e6, 1.0e7)}
