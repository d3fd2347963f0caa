"""The oracle of tests/test_gpu_binned.py: the cells of mdb_binned_buckets* from the oracle's grids of two fields of
tests/comoments_cases.py - the pairs and buckets of comoments_cases.oracle, the cell of the x value by its totalOrder
key (np.searchsorted(edge keys, key, side="right"): the number of edges at or below it), and per cell the count and, in
exact arithmetic (math.fsum around the cell's first value, as comoments_cases.cell_reference), the mean and m2 of y. It
also records the largest |y| of the cell, whether every y is finite, the number of x segments that feed the cell and
the number of runs, of the cell and of the call: maximal stretches of consecutive pairs of one x segment in one bucket and one cell."""

import math

import numpy as np

import comoments_cases as cc
import modelardb_rs_amd as mdb

I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
MEAN_TOLERANCE = cc.MEAN_TOLERANCE   # of the cell's largest |y|
M2_TOLERANCE = cc.M2_TOLERANCE       # of m2_ref
CELL = mdb.MOMENTS_CELL_DTYPE


def keys_of(values):
    """IEEE 754 totalOrder of f32 values as signed integers."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.int64)
    signed = np.where(bits >= 1 << 31, bits - (1 << 32), bits)
    return np.where(signed < 0, signed ^ 0x7FFFFFFF, signed)


def cells_of(values, edges):
    return np.searchsorted(keys_of(edges), keys_of(values), side="right")


def quantile_edges(values, n_edges):
    """n_edges quantiles of the finite values, as distinct f32 in ascending order (fewer where quantiles coincide)."""
    finite = values[np.isfinite(values)].astype(np.float64)
    edges = np.quantile(finite, np.linspace(0.0, 1.0, n_edges + 2)[1:-1]).astype(np.float32)
    return np.unique(edges)


def y_reference(y):
    """(mean, m2) of the f32 values of one cell, in exact arithmetic."""
    d = y.astype(np.float64) - float(y[0])
    shift = math.fsum(d) / len(d)
    r = d - shift
    return float(y[0]) + shift, math.fsum(r * r)


def oracle(x, y, edges, groups, n_groups, origin, width, n_buckets, t_lo=I64_MIN, t_hi=I64_MAX):
    keep_x, keep_y = x.in_range(t_lo, t_hi), y.in_range(t_lo, t_hi)
    assert int(keep_x.sum()) == int(keep_y.sum())
    ts, xv, yv, segment = x.ts[keep_x], x.values[keep_x], y.values[keep_y], x.segment[keep_x]
    groups = np.zeros(len(x.batch), dtype=np.uint32) if groups is None else groups
    point_groups = groups.astype(np.int64)[segment]
    buckets = cc._point_buckets(ts, origin, width)
    keep = (buckets >= 0) & (buckets < n_buckets)
    rows = np.flatnonzero(keep)
    n_value_cells = len(edges) + 1
    value_cells = cells_of(xv[keep], edges)
    cells = (point_groups[keep] * n_buckets + buckets[keep]) * n_value_cells + value_cells
    segment, yv = segment[keep], yv[keep]
    n_cells = n_groups * n_buckets * n_value_cells
    out = {"count": np.zeros(n_cells, dtype=np.int64), "mean": np.zeros(n_cells), "m2": np.zeros(n_cells),
           "largest": np.zeros(n_cells), "finite": np.ones(n_cells, dtype=bool),
           "segments": np.zeros(n_cells, dtype=np.int64), "cell_runs": np.zeros(n_cells, dtype=np.int64)}
    runs = 0
    if len(cells):
        new_run = np.concatenate([[True], (cells[1:] != cells[:-1]) | (segment[1:] != segment[:-1])
                                  | (rows[1:] != rows[:-1] + 1)])
        runs = int(new_run.sum())
        out["cell_runs"] = np.bincount(cells[new_run], minlength=n_cells).astype(np.int64)
        order = np.argsort(cells, kind="stable")
        sorted_cells, ys, segments = cells[order], yv[order], segment[order]
        starts = np.flatnonzero(np.concatenate([[True], sorted_cells[1:] != sorted_cells[:-1]]))
        ends = np.concatenate([starts[1:], [len(cells)]])
        with np.errstate(invalid="ignore", over="ignore"):
            for start, end in zip(starts, ends):
                cell, run = sorted_cells[start], ys[start:end]
                out["count"][cell] = end - start
                out["segments"][cell] = len(np.unique(segments[start:end]))
                out["finite"][cell] = bool(np.isfinite(run).all())
                if out["finite"][cell]:
                    out["mean"][cell], out["m2"][cell] = y_reference(run)
                    out["largest"][cell] = float(np.abs(run.astype(np.float64)).max())
    out = {name: array.reshape(n_groups, n_buckets, n_value_cells) for name, array in out.items()}
    out["runs"] = runs
    return out


WORST = {"mean": 0.0, "m2": 0.0}   # the largest ratios any call of assert_cells has seen


def assert_cells(got, expected, context="", fresh=True):
    """count exact; in a cell of finite y the mean within 2^-44 of the cell's largest |y|, m2 within 1e-5 of its
    reference and not negative; in a cell with a non-finite y neither is finite. `fresh`: the call began with fresh
    cells, so a cell without pairs is all-zero bytes still. Prints the worst ratios."""
    assert got.shape == expected["count"].shape and got.dtype == CELL, context
    np.testing.assert_array_equal(got["count"], expected["count"], err_msg=context)
    hit = expected["count"] > 0
    if fresh:
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * CELL.itemsize), context
    special = hit & ~expected["finite"]
    assert not np.isfinite(got["mean"][special]).any() and not np.isfinite(got["m2"][special]).any(), context
    plain = hit & expected["finite"]
    assert np.isfinite(got["mean"][plain]).all() and np.isfinite(got["m2"][plain]).all(), context
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_error = np.abs(got["mean"][plain] - expected["mean"][plain])
        m2_error = np.abs(got["m2"][plain] - expected["m2"][plain])
        worst_mean = np.nan_to_num(mean_error / expected["largest"][plain]).max(initial=0.0)
        worst_m2 = np.nan_to_num(m2_error / expected["m2"][plain]).max(initial=0.0)
    WORST["mean"], WORST["m2"] = max(WORST["mean"], worst_mean), max(WORST["m2"], worst_m2)
    print(f"{context}: {int(plain.sum())} cells, {expected['runs']} runs, mean error / max|y| <= {worst_mean:.3g} (allowed "
          f"{MEAN_TOLERANCE:.3g}), m2 error / m2 <= {worst_m2:.3g} (allowed {M2_TOLERANCE:.3g}); so far {WORST['mean']:.3g}, "
          f"{WORST['m2']:.3g}")
    assert (mean_error <= MEAN_TOLERANCE * expected["largest"][plain]).all(), (context, "mean")
    assert (m2_error <= M2_TOLERANCE * expected["m2"][plain]).all(), (context, "m2")   # (m2_ref == 0: 0.0)
    assert (got["m2"][plain] >= 0.0).all(), (context, "m2 >= 0")
