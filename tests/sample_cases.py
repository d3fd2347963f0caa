"""The reference of tests/test_gpu_sample.py and tests/test_sample_cpu.py: the cells of mdb_sample_at* for one field
of tests/comoments_cases.py's tables, from the oracle's grid of the field (Field.ts / Field.values / Field.segment).
The linked rule is applied row by row; rule (a) - a row on an instant contributes its value - and rule (b) - a linked
interval around an instant contributes f(T) - are applied in fractions.Fraction over Python integers, so the
reference has no error of its own. Nothing here calls the library under test.

f(T) on the linked interval (t0, v0) - (t1, v1), t0 < T < t1:
  STEP    v0
  LINEAR  v0 + (v1 - v0) * (T - t0) / (t1 - t0)
  EXACT   no contribution between rows
The tolerance of a cell is 2^-48 * sum max(|v0|, |v1|) over its contributions (a row: |v|), the contract's, which the
contract derives from the roundings of one contribution and of the additions."""

import math
from fractions import Fraction

import numpy as np

import comoments_cases as cc

LINEAR, STEP, EXACT = 0, 1, 2
METHODS = ((LINEAR, "linear"), (STEP, "step"), (EXACT, "exact"))
I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
INTERVAL = cc.INTERVAL
TOLERANCE = Fraction(1, 1 << 48)
CELL_DTYPE = np.dtype([("count", "<u8"), ("sum", "<f8")])


def _instants_between(origin, width, n_instants, lo, hi):
    """The k < n_instants with lo <= origin + k * width <= hi, as a range."""
    first = max(0, -((origin - lo) // width))   # ceil((lo - origin) / width)
    last = min(n_instants - 1, (hi - origin) // width)
    return range(first, last + 1)


def sample_rows(timestamps, values, row_groups, n_groups, origin, width, n_instants, method, max_gap=None):
    """The cells of the rows (timestamps, values, row_groups), in row order: a dict of (n_groups, n_instants) arrays -
    count (exact), sum (object array of Fractions: the exact sum of the finite contributions; 0 where `finite` is
    False), scale (object array of Fractions: the tolerance's sum), finite (no contribution of the cell reads a
    non-finite value)."""
    ts = [int(t) for t in timestamps]
    vs = [float(v) for v in values]
    gs = [int(g) for g in row_groups]
    n_cells = n_groups * n_instants
    count = [0] * n_cells
    total = [Fraction(0)] * n_cells
    scale = [Fraction(0)] * n_cells
    finite = [True] * n_cells

    def contribute(cell, value, magnitude):
        count[cell] += 1
        if value is None:
            finite[cell] = False
        else:
            total[cell] += value
            scale[cell] += magnitude

    for r, (t, v, g) in enumerate(zip(ts, vs, gs)):
        # (a) the row itself
        if t >= origin and (t - origin) % width == 0 and (t - origin) // width < n_instants:
            contribute(g * n_instants + (t - origin) // width, Fraction(v) if math.isfinite(v) else None,
                       Fraction(abs(v)) if math.isfinite(v) else None)
        # (b) the linked interval to the next row
        if method == EXACT or r + 1 == len(ts):
            continue
        t1, v1 = ts[r + 1], vs[r + 1]
        if gs[r + 1] != g or t1 <= t or (max_gap is not None and t1 - t > max_gap):
            continue
        for k in _instants_between(origin, width, n_instants, t + 1, t1 - 1):
            at = origin + k * width
            if method == STEP or v == v1:
                ok = math.isfinite(v)
                value = Fraction(v) if ok else None
            else:
                ok = math.isfinite(v) and math.isfinite(v1)
                value = Fraction(v) + (Fraction(v1) - Fraction(v)) * Fraction(at - t, t1 - t) if ok else None
            if ok:
                magnitude = Fraction(max(abs(v), abs(v1) if math.isfinite(v1) else abs(v)))
            else:
                magnitude = None
            contribute(g * n_instants + k, value, magnitude)
    shape = (n_groups, n_instants)
    as_objects = lambda items: np.array(items + [None], dtype=object)[:-1].reshape(shape)
    return {
        "count": np.array(count, dtype=np.uint64).reshape(shape),
        "sum": as_objects([s if ok else Fraction(0) for s, ok in zip(total, finite)]),
        "scale": as_objects(scale),
        "finite": np.array(finite, dtype=bool).reshape(shape),
    }


def oracle(field, groups, n_groups, origin, width, n_instants, method, max_gap=None):
    """sample_rows of a comoments_cases.Field; groups: per segment, or None (every segment in group 0)."""
    segment_groups = np.zeros(len(field.batch), dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    return sample_rows(field.ts, field.values, segment_groups[field.segment], n_groups, origin, width, n_instants,
                       method, max_gap)


def values_of(expected):
    """sum / count of the reference as float64 (correctly rounded), NaN where count == 0 or the cell is not finite."""
    out = np.full(expected["count"].shape, np.nan)
    for index in np.ndindex(*out.shape):
        if expected["count"][index] > 0 and expected["finite"][index]:
            out[index] = float(expected["sum"][index] / int(expected["count"][index]))
    return out


def assert_cells(got, expected, context="", fresh=True):
    """count equal in every cell; the sum not finite exactly where the reference says so (for a cell with
    contributions) and within TOLERANCE * scale of the exact sum everywhere else, compared in exact arithmetic.
    `fresh`: the call began with fresh cells, so a cell without a contribution is all-zero bytes still. Prints the
    worst ratio. Returns (plain, special): how many cells of each kind."""
    assert got.shape == expected["count"].shape, context
    np.testing.assert_array_equal(got["count"], expected["count"], err_msg=context)
    hit = expected["count"] > 0
    if fresh:
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * CELL_DTYPE.itemsize), context
    special = hit & ~expected["finite"]
    plain = hit & expected["finite"]
    assert not np.isfinite(got["sum"][special]).any(), context
    assert np.isfinite(got["sum"][plain]).all(), context
    worst = Fraction(0)
    for index in zip(*np.nonzero(plain)):
        error = abs(Fraction(float(got["sum"][index])) - expected["sum"][index])
        allowed = TOLERANCE * expected["scale"][index]
        if expected["scale"][index] > 0:
            worst = max(worst, error / expected["scale"][index])
        assert error <= allowed, (context, index, float(error), float(allowed))
    print(f"{context}: {int(plain.sum())} cells ({int(special.sum())} not finite), sum error / scale <= "
          f"{float(worst):.3g} (allowed {float(TOLERANCE):.3g})")
    return int(plain.sum()), int(special.sum())
