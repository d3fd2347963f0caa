"""The reference of tests/test_gpu_change.py: the cells of mdb_change_buckets* for one field of
tests/comoments_cases.py's tables, from the oracle's grid of the field (Field.ts / Field.values / Field.segment). The
linked rule is integral_cases.linked_intervals'; every linked pair is assigned to the bucket of its later row in
Python integers; d is the numpy float64 difference of the two float32 values (one rounding, as the contract forms it).
Integers are exact, the maxima are exact (a maximum of individually rounded differences), the three sums are
math.fsum of their terms. Nothing here calls the library under test.

Per cell the reference also keeps S, the sum of the magnitudes of each sum's terms, for the contract's tolerance
|got - exact| <= count * 2^-52 * S, and `poisoned`: a pair of the cell has d NaN (a NaN value, or inf - inf), which
makes rise and fall NaN and leaves the other members alone."""

import math

import numpy as np

import comoments_cases as cc
import integral_cases as ic

I64_MIN, I64_MAX = cc.I64_MIN, cc.I64_MAX
INTERVAL = cc.INTERVAL
EPSILON = 2.0 ** -52
CELL_DTYPE = np.dtype([("count", "<u8"), ("n_fall", "<u8"), ("duration", "<u8"), ("rise", "<f8"), ("fall", "<f8"),
                       ("reset_sum", "<f8"), ("max_rise", "<f8"), ("max_fall", "<f8")])
EXACT = ("count", "n_fall", "duration", "max_rise", "max_fall")
SUMS = ("rise", "fall", "reset_sum")


def cells_of(intervals, n_groups, origin, width, n_buckets):
    """The cells of the linked pairs [(t0, v0, t1, v1, group)]: a dict of (n_groups, n_buckets) arrays - the eight
    members, `scale_<sum>` (S of each sum) and `poisoned`."""
    n_cells = n_groups * n_buckets
    count, n_fall, duration = [0] * n_cells, [0] * n_cells, [0] * n_cells
    terms = {name: [[] for _ in range(n_cells)] for name in SUMS}
    max_rise, max_fall = [0.0] * n_cells, [0.0] * n_cells
    poisoned = [False] * n_cells
    for t0, v0, t1, v1, group in intervals:
        if t1 < origin or t1 >= origin + n_buckets * width:
            continue
        cell = group * n_buckets + (t1 - origin) // width
        with np.errstate(invalid="ignore"):   # (inf - inf is a NaN the contract names, not a mistake)
            d = float(np.float64(np.float32(v1)) - np.float64(np.float32(v0)))
        count[cell] += 1
        duration[cell] += t1 - t0
        if d > 0:
            terms["rise"][cell].append(d)
            max_rise[cell] = max(max_rise[cell], d)
        elif d < 0:
            n_fall[cell] += 1
            terms["fall"][cell].append(-d)
            terms["reset_sum"][cell].append(float(v1))
            max_fall[cell] = max(max_fall[cell], -d)
        elif d != d:
            poisoned[cell] = True
    shape = (n_groups, n_buckets)

    def total(values):
        finite = [v for v in values if math.isfinite(v)]
        if len(finite) != len(values):   # an infinite term: the sum is that infinity (they never cancel: see below)
            signs = {v for v in values if not math.isfinite(v)}
            assert len(signs) == 1
            return signs.pop()
        return math.fsum(values)

    out = {
        "count": np.array(count, dtype=np.uint64).reshape(shape),
        "n_fall": np.array(n_fall, dtype=np.uint64).reshape(shape),
        "duration": np.array([d % (1 << 64) for d in duration], dtype=np.uint64).reshape(shape),
        "max_rise": np.array(max_rise).reshape(shape),
        "max_fall": np.array(max_fall).reshape(shape),
        "poisoned": np.array(poisoned, dtype=bool).reshape(shape),
    }
    for name in SUMS:   # (rise and fall have positive terms only; reset_sum's infinite terms are all -inf)
        out[name] = np.array([total(t) for t in terms[name]]).reshape(shape)
        out["scale_" + name] = np.array([total([abs(v) for v in t]) for t in terms[name]]).reshape(shape)
    return out


def oracle(field, groups, n_groups, origin, width, n_buckets, max_gap=None):
    return cells_of(ic.field_intervals(field, groups, max_gap), n_groups, origin, width, n_buckets)


def rows_oracle(timestamps, values, n_buckets, origin, width, max_gap=None):
    """One group, the rows given directly."""
    intervals = ic.linked_intervals(timestamps, values, np.zeros(len(timestamps), dtype=np.int64), max_gap)
    return cells_of(intervals, 1, origin, width, n_buckets)


def assert_cells(got, expected, context="", fresh=True):
    """The five exact members equal in every cell; rise / fall NaN exactly where the reference says poisoned; the
    three sums within count * 2^-52 * S elsewhere (an infinite S: the same infinity); `fresh`: the call began with
    fresh cells, so a cell without a pair is all-zero bytes still. Prints the worst ratio error / (count * 2^-52 * S).
    Returns (plain, poisoned): how many cells with pairs of each kind."""
    assert got.dtype == CELL_DTYPE and got.shape == expected["count"].shape, context
    for name in EXACT:
        np.testing.assert_array_equal(got[name], expected[name], err_msg=f"{context}: {name}")
    hit = expected["count"] > 0
    if fresh:
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * CELL_DTYPE.itemsize), context
    poisoned = expected["poisoned"]
    assert not (poisoned & ~hit).any()
    worst = 0.0
    for name in SUMS:
        checked = hit if name == "reset_sum" else hit & ~poisoned
        if name != "reset_sum":
            assert np.isnan(got[name][poisoned]).all(), f"{context}: {name} not NaN in a poisoned cell"
        assert not np.isnan(got[name][checked]).any(), f"{context}: {name} NaN in a cell that is not poisoned"
        value, reference, scale = got[name][checked], expected[name][checked], expected["scale_" + name][checked]
        pairs = expected["count"][checked].astype(np.float64)
        infinite = np.isinf(scale)
        np.testing.assert_array_equal(value[infinite], reference[infinite], err_msg=f"{context}: {name}")
        error = np.abs(value[~infinite] - reference[~infinite])
        allowed = pairs[~infinite] * EPSILON * scale[~infinite]
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, np.nan_to_num(error / allowed).max(initial=0.0))
        assert (error <= allowed).all(), f"{context}: {name} off by up to {np.nan_to_num(error / allowed).max():.3g} x allowed"
    print(f"{context}: {int((hit & ~poisoned).sum())} cells ({int(poisoned.sum())} poisoned), "
          f"sum error / (count * 2^-52 * S) <= {worst:.3g} (allowed 1)")
    return int((hit & ~poisoned).sum()), int(poisoned.sum())
