"""The reference of tests/test_gpu_moments.py: ora.grid_batch's points put into cells as tests/m4_cases.py does, and per
cell in exact arithmetic (math.fsum): d = v - v[0] in f64, mean_ref = v[0] + fsum(d) / n, m2_ref = fsum((d - fsum(d) / n)^2).
Tolerances: count exact; |mean - mean_ref| <= 2^-44 * max|v| of the cell; |m2 - m2_ref| <= 1e-5 * m2_ref; in a cell
that holds a NaN or an infinity neither mean nor m2 is finite. Nothing here calls the library under test."""

import math

import numpy as np

import oracle_lib as ora
import modelardb_rs_amd as mdb

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MEAN_TOLERANCE = 2.0 ** -44   # of the largest |v| of the cell
M2_TOLERANCE = 1e-5           # of m2_ref


def point_buckets(timestamps, origin, width):
    """floor((t - origin) / width) per point as int64 where that fits (-1: below bucket 0 or beyond int64)."""
    if len(timestamps) == 0:
        return np.zeros(0, dtype=np.int64)
    lo, hi = int(timestamps.min()) - origin, int(timestamps.max()) - origin
    if I64_MIN <= lo and hi <= I64_MAX:
        return (timestamps - np.int64(origin)) // np.int64(width)
    buckets = [(int(t) - origin) // width for t in timestamps]
    return np.array([b if 0 <= b <= I64_MAX else -1 for b in buckets], dtype=np.int64)


GRIDS = {}


def grid(batch):
    """ora.grid_batch(batch), computed once per batch object."""
    if id(batch) not in GRIDS:
        timestamps, values, rows, _ = ora.grid_batch(batch)
        GRIDS[id(batch)] = (batch, timestamps.astype(np.int64), values.astype(np.float32), rows.astype(np.int64))
    return GRIDS[id(batch)][1:]


def cell_reference(values):
    """(mean_ref, m2_ref) of the f32 values of one cell, in exact arithmetic."""
    d = values.astype(np.float64) - float(values[0])
    shift = math.fsum(d) / len(d)
    return float(values[0]) + shift, math.fsum((d - shift) ** 2)


def reduce(values, cells, n_cells):
    """count, mean_ref, m2_ref, the largest |v| and "every point finite" per cell, over points that carry their cell
    number."""
    out = {"count": np.zeros(n_cells, dtype=np.int64), "mean": np.zeros(n_cells), "m2": np.zeros(n_cells),
           "largest": np.zeros(n_cells), "finite": np.ones(n_cells, dtype=bool)}
    if len(cells) == 0:
        return out
    order = np.argsort(cells, kind="stable")
    sorted_cells, sorted_values = cells[order], values[order]
    starts = np.flatnonzero(np.concatenate([[True], sorted_cells[1:] != sorted_cells[:-1]]))
    ends = np.concatenate([starts[1:], [len(cells)]])
    with np.errstate(invalid="ignore", over="ignore"):
        for start, end in zip(starts, ends):
            cell, run = sorted_cells[start], sorted_values[start:end]
            out["count"][cell] = end - start
            out["finite"][cell] = bool(np.isfinite(run).all())
            if out["finite"][cell]:
                out["mean"][cell], out["m2"][cell] = cell_reference(run)
                out["largest"][cell] = float(np.abs(run.astype(np.float64)).max())
    return out


def oracle(batch, groups, n_groups, origin, width, n_buckets, t_lo=I64_MIN, t_hi=I64_MAX):
    timestamps, values, rows = grid(batch)
    groups = np.zeros(len(batch), dtype=np.uint32) if groups is None else groups
    point_groups = np.repeat(groups.astype(np.int64), rows)
    buckets = point_buckets(timestamps, origin, width)
    keep = (timestamps >= t_lo) & (timestamps <= t_hi) & (buckets >= 0) & (buckets < n_buckets)
    cells = point_groups[keep] * n_buckets + buckets[keep]
    reduced = reduce(values[keep], cells, n_groups * n_buckets)
    return {name: array.reshape(n_groups, n_buckets) for name, array in reduced.items()}


def assert_cells(got, expected, context="", fresh=True):
    """count exact, mean and m2 within the tolerances of the module's docstring; `fresh`: the call began with fresh
    cells, so a cell without points is all-zero bytes still."""
    assert got.shape == expected["count"].shape, context
    np.testing.assert_array_equal(got["count"], expected["count"], err_msg=context)
    hit = expected["count"] > 0
    if fresh:
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * mdb.MOMENTS_CELL_DTYPE.itemsize), context
    special = hit & ~expected["finite"]
    assert not np.isfinite(got["mean"][special]).any() and not np.isfinite(got["m2"][special]).any(), context
    plain = hit & expected["finite"]
    mean_error = np.abs(got["mean"][plain] - expected["mean"][plain])
    m2_error = np.abs(got["m2"][plain] - expected["m2"][plain])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_ratio = np.nan_to_num(mean_error / expected["largest"][plain])
        m2_ratio = np.nan_to_num(m2_error / expected["m2"][plain])
    print(f"{context}: {int(plain.sum())} cells, mean error / max|v| <= {mean_ratio.max(initial=0.0):.3g} "
          f"(allowed {MEAN_TOLERANCE:.3g}), m2 error / m2 <= {m2_ratio.max(initial=0.0):.3g} (allowed {M2_TOLERANCE:.3g})")
    assert np.isfinite(got["mean"][plain]).all() and np.isfinite(got["m2"][plain]).all(), context
    assert (mean_error <= MEAN_TOLERANCE * expected["largest"][plain]).all(), context
    assert (m2_error <= M2_TOLERANCE * expected["m2"][plain]).all(), context   # (m2_ref == 0: m2 == 0.0)
    assert (got["m2"][plain] >= 0.0).all(), context
