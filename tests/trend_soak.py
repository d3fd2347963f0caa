"""Cases and the point-by-point reference of the trend operator's soak (a helper module: tests/test_gpu_trend_soak.py runs
the cases on the GPU, tests/test_trend_soak_cpu.py keeps them honest, tests/shard_soak.py cuts them into shards).

draw(index) takes tests/query_soak.py's case `index` and adds two requests that put the ORIGIN where the x arithmetic
can go wrong; reference(case, request) is point by point: x = (t - origin) - bucket * width in integers, dx = x - x_first
(an integer below 2^53), each cell in exact arithmetic (comoments_cases.cell_reference on (dx, v), math.fsum). Nothing here
calls the library under test."""

from types import SimpleNamespace

import numpy as np

import comoments_cases as cc
import query_soak as qs

N_CASES = 200
SEED = 0x5452454E
I64_MIN, I64_MAX = qs.I64_MIN, qs.I64_MAX
FAR_WIDTHS = ((1 << 41) + 1, (1 << 54) + 3, (1 << 62) + 5, I64_MAX)


def draw(index):
    """(case, requests): query_soak's case `index`, its requests and the hostile ones, a pure function of `index`."""
    case = qs.make_case(index)
    rng = np.random.default_rng([SEED, index])
    first = int(case.timestamps.min())
    requests = list(case.requests)
    # the origin far below the data: the data in bucket 0 or 1 of very wide buckets
    width = int(FAR_WIDTHS[int(rng.integers(0, len(FAR_WIDTHS)))])
    ahead = int(rng.integers(0, 2))
    origin = max(first - ahead * width - int(rng.integers(0, 1 << 20)), I64_MIN)
    requests.append(SimpleNamespace(style="far", origin=origin, width=width, n_buckets=ahead + 2, t_lo=None, t_hi=None))
    # the origin a microsecond either side of a timestamp, narrow buckets: x of 0, 1 and width - 1
    at = int(case.timestamps[int(rng.integers(0, len(case.timestamps)))])
    width = int(rng.choice([1, 2, 1000, 60_000_000]))
    requests.append(SimpleNamespace(style="near", origin=at + int(rng.integers(-1, 2)), width=width,
                                    n_buckets=int(rng.choice([1, 64, qs.MAX_CELLS // 4])), t_lo=None, t_hi=None))
    return case, requests


def reference(case, request):
    """The cells of a request in the shape comoments_cases.assert_cells takes, point by point with integers for x."""
    inside, cells = qs.place(case, request)
    timestamps, values = case.timestamps[inside], case.values[inside]
    n_cells = case.n_groups * request.n_buckets
    out = {"count": np.zeros(n_cells, dtype=np.int64), "largest_x": np.zeros(n_cells), "largest_y": np.zeros(n_cells),
           "finite_x": np.ones(n_cells, dtype=bool), "finite_y": np.ones(n_cells, dtype=bool)}
    out.update({name: np.zeros(n_cells) for name in cc.MEMBERS})
    if len(cells):
        order = np.argsort(cells, kind="stable")
        sorted_cells, ts, ys = cells[order], timestamps[order], values[order]
        starts = np.flatnonzero(np.concatenate([[True], sorted_cells[1:] != sorted_cells[:-1]]))
        ends = np.concatenate([starts[1:], [len(cells)]])
        with np.errstate(invalid="ignore", over="ignore"):
            for start, end in zip(starts, ends):
                cell, run_y = int(sorted_cells[start]), ys[start:end]
                bucket = cell % request.n_buckets
                x = [(int(t) - request.origin) - bucket * request.width for t in ts[start:end]]   # Python integers
                assert 0 <= min(x) and max(x) < request.width
                dx = np.array([value - x[0] for value in x], dtype=np.float64)
                assert max(abs(value - x[0]) for value in x) < 1 << 53   # (dx is exact)
                out["count"][cell] = end - start
                out["finite_y"][cell] = bool(np.isfinite(run_y).all())
                if out["finite_y"][cell]:
                    shift_x, mean_y, m2_x, m2_y, c_xy = cc.cell_reference(dx, run_y)
                    out["mean_x"][cell], out["mean_y"][cell] = float(x[0] + shift_x), mean_y
                    out["m2_x"][cell], out["m2_y"][cell], out["c_xy"][cell] = m2_x, m2_y, c_xy
                    out["largest_x"][cell] = float(max(x))
                    out["largest_y"][cell] = float(np.abs(run_y.astype(np.float64)).max())
    return {name: array.reshape(case.n_groups, request.n_buckets) for name, array in out.items()}
