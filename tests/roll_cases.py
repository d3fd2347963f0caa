"""The reference of tests/test_roll_cpu.py and tests/test_gpu_roll.py: the rule of mdb_roll_cells* (include/mdb.h)
restated in Python over the EXISTING merge wrappers (agg_merge_n, m4_merge, moments_merge, comoments_merge,
derived_merge, integral_merge, change_merge; numpy's wrapping add for uint64), applied in exactly the stated order, and
generators of random cells per kind. Nothing here calls mdb_roll_*.

The rule, with m = window and blocks of m buckets aligned at multiples of m from bucket 0:
    P[b] = cell[b] where b % m == 0, else merge(into = P[b-1], from = cell[b])
    S[b] = cell[b] where b % m == m - 1, else merge(into = a copy of cell[b], from = S[b+1])
    window k starts at a = k * stride:  a % m == 0: P[a+m-1];  otherwise merge(into = S[a], from = P[a+m-1])
(P[a+m-1] is P_{j+1}[r-1] for a = j * m + r.) The merges run on whole [n_outer][n_inner] slabs at once: columns never
meet."""

import functools

import numpy as np

import modelardb_rs_amd as mdb

FLT_MAX = np.float32(3.4028234663852886e38)
KINDS = {"agg": mdb.MDB_ROLL_AGG, "m4": mdb.MDB_ROLL_M4, "moments": mdb.MDB_ROLL_MOMENTS,
         "comoments": mdb.MDB_ROLL_COMOMENTS, "derived": mdb.MDB_ROLL_DERIVED, "integral": mdb.MDB_ROLL_INTEGRAL,
         "change": mdb.MDB_ROLL_CHANGE, "u64": mdb.MDB_ROLL_U64}
CELL_SIZES = {"agg": 24, "m4": 56, "moments": 24, "comoments": 48, "derived": 32, "integral": 16, "change": 64, "u64": 8}


def _add_u64(into, from_):
    with np.errstate(over="ignore"):
        into += from_
    return into


MERGES = {"agg": mdb.agg_merge_n, "m4": mdb.m4_merge, "moments": mdb.moments_merge, "comoments": mdb.comoments_merge,
          "derived": mdb.derived_merge, "integral": mdb.integral_merge, "change": mdb.change_merge, "u64": _add_u64}


def dtype_of(kind):
    return mdb.ROLL_KINDS[KINDS[kind]]


def merged(kind, into, from_):
    """A new array: merge(into = a copy of `into`, from = `from_`), element for element."""
    out = np.ascontiguousarray(into).copy()
    if out.size:
        MERGES[kind](out.reshape(-1), np.ascontiguousarray(from_).reshape(-1))
    return out


def image(kind, cells):
    """The bytes of `cells` - for the kinds whose merge computes with floats, with every NaN member replaced by one
    NaN (M4 only selects and uint64 only adds integers: their bytes are compared as they are): what two forms are
    compared by. The merge rules
    leave the sign and the payload of a NaN they produce or pass on to the instruction that adds or multiplies (x86
    makes 0xFFF8... of inf - inf where gfx950 makes 0x7FF8..., and of two NaN operands either may come out, by the
    order the compiler gave them), so those bits are no part of what mdb_roll_cells* promises; that the member IS a NaN,
    and every other bit of every cell, is."""
    cells = np.ascontiguousarray(cells).copy()
    if kind in ("m4", "u64"):
        return cells.tobytes()
    for name in cells.dtype.names:
        if cells.dtype[name].kind == "f":
            member = cells[name]
            member[np.isnan(member)] = np.nan
    return cells.tobytes()


def n_windows_of(n_buckets, window, stride):
    return 0 if n_buckets < window else (n_buckets - window) // stride + 1


def folds(kind, cells, window):
    """(P, S) of cells [n_outer][n_buckets][n_inner], both of the cells' shape. S of a last, partial block is not
    formed (no window reads it): it stays a copy of the cells."""
    n_buckets, m = cells.shape[1], window
    prefix, suffix = cells.copy(), cells.copy()
    for b in range(n_buckets):
        if b % m != 0:
            prefix[:, b] = merged(kind, prefix[:, b - 1], cells[:, b])
    whole = (n_buckets // m) * m
    for b in range(whole - 1, -1, -1):
        if b % m != m - 1:
            suffix[:, b] = merged(kind, cells[:, b], suffix[:, b + 1])
    return prefix, suffix


def windows_from(kind, prefix, suffix, window, stride):
    """The windows [n_outer][n_windows][n_inner] from the two folds."""
    n_outer, n_buckets, n_inner = prefix.shape
    n_windows = n_windows_of(n_buckets, window, stride)
    starts = np.arange(n_windows, dtype=np.int64) * stride
    out = np.ascontiguousarray(prefix[:, starts + window - 1]) if n_windows else prefix[:, :0].copy()
    inside = np.flatnonzero(starts % window != 0)
    if len(inside):
        out[:, inside] = merged(kind, suffix[:, starts[inside]], prefix[:, starts[inside] + window - 1])
    return out.reshape(n_outer, n_windows, n_inner)


def reference(kind, cells, window, stride):
    prefix, suffix = folds(kind, cells, window)
    return windows_from(kind, prefix, suffix, window, stride)


def left_fold(kind, cells, start, window):
    """cell[start] with cell[start+1] .. cell[start+window-1] merged in, one after the other: chained *_merge_n."""
    into = np.ascontiguousarray(cells[:, start]).copy()
    for b in range(start + 1, start + window):
        into = merged(kind, into, cells[:, b])
    return into


def _garbage(rng, cells, empty, share=0.5):
    """Of the empty cells (count == 0) a share gets 0xA5 in every member but count."""
    flat = cells.reshape(-1)
    picked = np.flatnonzero(empty.reshape(-1) & (rng.random(flat.size) < share))
    raw = flat.view(np.uint8).reshape(flat.size, cells.dtype.itemsize)
    raw[picked] = 0xA5
    flat["count"][picked] = 0


def _floats(rng, shape, dtype=np.float32):
    """Random values around a few levels with +-0, and a few huge ones."""
    values = (rng.choice([0.0, 1.0, 1.0e6], shape) + rng.normal(0.0, 0.5, shape)).astype(dtype)
    zero = rng.random(shape) < 0.15
    values[zero] = np.where(rng.random(shape) < 0.5, 0.0, -0.0).astype(dtype)[zero]
    return values


def random_cells(kind, shape, seed=0):
    """Random cells of `kind` [n_outer][n_buckets][n_inner]: empty cells sprinkled in, count == 0 cells with 0xA5
    garbage in the other members, +-0 extremes, NaN-only cells (FLT_MAX / -FLT_MAX) and non-finite means."""
    rng = np.random.default_rng([seed, KINDS[kind]])
    cells = np.zeros(shape, dtype=dtype_of(kind))
    if kind == "u64":
        cells[...] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
        cells[rng.random(shape) < 0.5] >>= np.uint64(40)
        return cells
    empty = rng.random(shape) < 0.25
    nan_only = ~empty & (rng.random(shape) < 0.08)
    count = np.where(empty, 0, rng.integers(1, 1000, shape))
    if kind != "integral":
        cells["count"] = count
    if kind == "agg":
        cells["sum"] = np.where(empty, 0.0, rng.normal(0.0, 1.0e3, shape))
        low, high = _floats(rng, shape), _floats(rng, shape)
        cells["min"], cells["max"] = np.minimum(low, high), np.maximum(low, high)
        cells["min"][empty | nan_only], cells["max"][empty | nan_only] = FLT_MAX, -FLT_MAX
        cells["sum"][nan_only] = np.nan
        odd = ~empty & (rng.random(shape) < 0.05)   # a NaN extreme, which the rule skips as `from` and replaces as `into`
        cells["min"][odd] = np.nan
    elif kind == "m4":
        base = rng.integers(0, 1000, shape) + np.arange(shape[1]).reshape(1, -1, 1) * 500   # (ties across buckets too)
        for name in ("t_first", "t_last", "t_min", "t_max"):
            cells[name] = base + rng.integers(0, 600, shape)
        for name in ("v_first", "v_last", "v_min", "v_max"):
            cells[name] = _floats(rng, shape)
            cells[name][nan_only] = np.nan
        flat = cells.reshape(-1)
        flat[empty.reshape(-1)] = np.zeros((), dtype=cells.dtype)
        _garbage(rng, cells, empty)
    elif kind in ("moments", "derived"):
        cells["mean"] = _floats(rng, shape, np.float64)
        cells["m2"] = np.abs(rng.normal(0.0, 10.0, shape))
        wild = ~empty & (rng.random(shape) < 0.08)
        cells["mean"][wild] = rng.choice([np.inf, -np.inf, np.nan], int(wild.sum()))
        cells["m2"][wild] = np.nan
        if kind == "derived":
            low, high = _floats(rng, shape), _floats(rng, shape)
            cells["min"], cells["max"] = np.minimum(low, high), np.maximum(low, high)
            cells["min"][nan_only], cells["max"][nan_only] = FLT_MAX, -FLT_MAX
            cells["mean"][nan_only] = cells["m2"][nan_only] = np.nan
        flat = cells.reshape(-1)
        flat[empty.reshape(-1)] = np.zeros((), dtype=cells.dtype)
        _garbage(rng, cells, empty)
    elif kind == "comoments":
        for name in ("mean_x", "mean_y"):
            cells[name] = _floats(rng, shape, np.float64)
        for name in ("m2_x", "m2_y"):
            cells[name] = np.abs(rng.normal(0.0, 10.0, shape))
        cells["c_xy"] = rng.normal(0.0, 5.0, shape)
        wild = ~empty & (rng.random(shape) < 0.08)
        cells["mean_x"][wild] = np.inf
        cells["m2_x"][wild] = cells["c_xy"][wild] = np.nan
        flat = cells.reshape(-1)
        flat[empty.reshape(-1)] = np.zeros((), dtype=cells.dtype)
        _garbage(rng, cells, empty)
    elif kind == "integral":
        cells["duration"] = np.where(empty, 0, rng.integers(0, 1 << 62, shape).astype(np.uint64))
        cells["integral"] = np.where(empty, 0.0, rng.normal(0.0, 1.0e9, shape))
        cells["integral"][nan_only] = rng.choice([np.inf, -np.inf, np.nan], int(nan_only.sum()))
    elif kind == "change":
        cells["n_fall"] = np.where(empty, 0, rng.integers(0, 1000, shape))
        cells["duration"] = np.where(empty, 0, rng.integers(0, 1 << 62, shape).astype(np.uint64))
        for name in ("rise", "fall", "reset_sum", "max_rise", "max_fall"):
            cells[name] = np.where(empty, 0.0, np.abs(rng.normal(0.0, 100.0, shape)))
        cells["rise"][nan_only] = cells["fall"][nan_only] = np.nan
    return cells


def m4_key(values):
    """The totalOrder key of float32 values (m4_key of mdb_m4.hpp)."""
    bits = np.asarray(values, dtype=np.float32).view(np.int32)
    return bits ^ ((bits >> 31) & np.int32(0x7FFFFFFF))


def m4_cell_of(timestamps, values):
    """The M4 cell of a set of points by the four rules of mdb.h, brute force."""
    cell = np.zeros((), dtype=mdb.M4_CELL_DTYPE)
    if len(timestamps) == 0:
        return cell
    keys = m4_key(values).astype(np.int64)
    points = list(zip(timestamps.tolist(), keys.tolist(), range(len(keys))))
    first = min(points, key=lambda p: (p[0], p[1]))
    last = max(points, key=lambda p: (p[0], p[1]))
    low = min(points, key=lambda p: (p[1], p[0]))
    high = min(points, key=lambda p: (-p[1], p[0]))
    cell["count"] = len(points)
    for name, point in (("first", first), ("last", last), ("min", low), ("max", high)):
        cell["t_" + name], cell["v_" + name] = point[0], values[point[2]]
    return cell


BIG = 200   # buckets of the arrays the cases of the shape grid are cut from


def shape_grid():
    """(window, stride, n_buckets): window in {1, 2, 3, 7, 64, 65, n_buckets}, stride in {1, 2, window, window + 1},
    n_buckets in {window, window + 1, 2 * window - 1, 200}; n_inner in {1, 3} and n_outer in {1, 5} are slices of big()."""
    cases = set()
    for window in (1, 2, 3, 7, 64, 65, BIG):   # (BIG: window = n_buckets of the largest array)
        for n_buckets in (window, window + 1, 2 * window - 1, BIG):
            if not window <= n_buckets <= BIG:
                continue
            for stride in (1, 2, window, window + 1):
                cases.add((window, stride, n_buckets))
    return sorted(cases)


@functools.lru_cache(maxsize=None)
def big(kind):
    """The random cells [5][BIG][3] of `kind` every case of the grid is cut from (made once, not to be written)."""
    cells = random_cells(kind, (5, BIG, 3), seed=2070)
    cells.setflags(write=False)
    return cells
