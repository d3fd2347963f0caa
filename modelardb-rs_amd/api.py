"""Thin Python binding of the C ABI in include/mdb.h (ctypes; no torch types cross the boundary).

``Context`` owns one ``mdb_ctx`` (one HIP stream + scratch). The host methods take numpy-backed
``SegmentBatch`` objects whose buffers are handed to the library as plain pointers, exactly like
the Rust shim in INTEGRATION.md would hand over Arrow buffers. There is no CPU fallback: if the HIP
library cannot be loaded or a call fails, ``HipError`` is raised.
"""

import ctypes as C
import struct
import time

import numpy as np

from . import _abi
from .segments import SegmentBatch


class HipError(RuntimeError):
    pass


class DeviceSegments:
    """A batch of segments resident in HBM (``mdb_segments_owned`` with on_device = 1)."""

    def __init__(self, context, pointer):
        self._context = context
        self.pointer = pointer

    def __len__(self):
        return int(self.pointer.contents.seg.n)

    @property
    def seg(self):
        return self.pointer.contents.seg

    def free(self):
        if self.pointer:
            self._context.lib.mdb_segments_free(self.pointer)
            self.pointer = None

    def download(self):
        """Copy back to the host as a ``SegmentBatch``."""
        out = C.POINTER(_abi.SegmentsOwnedC)()
        self._context._check(self._context.lib.mdb_segments_download(
            self._context.handle, self.pointer, C.byref(out)))
        try:
            return SegmentBatch.from_owned(out)
        finally:
            self._context.lib.mdb_segments_free(out)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GridTicket:
    """An outstanding mdb_grid_submit. wait() returns (timestamps, values, rows_per_segment, metrics,
    tag_views) as copies ((n, 16) uint8 arrays for the tag views) and consumes the ticket."""

    def __init__(self, context, pointer, keep, n_tags, values_only):
        self._context, self._pointer, self._keep = context, pointer, keep
        self._n_tags, self._values_only = n_tags, values_only

    def wait(self):
        context, pointer = self._context, self._pointer
        self._pointer = None
        out = C.POINTER(_abi.GridResultC)()
        context._check(context.lib.mdb_grid_wait(pointer, C.byref(out)))
        self._keep = None
        result = out.contents
        n, n_segments = int(result.n), int(result.n_segments)

        def copy_of(pointer, count, dtype, width=1):
            if count == 0:
                return np.zeros((0, width) if width > 1 else 0, dtype=dtype)
            nbytes = count * width * np.dtype(dtype).itemsize
            array = np.frombuffer((C.c_char * nbytes).from_address(pointer), dtype=dtype).copy()
            return array.reshape(count, width) if width > 1 else array

        try:
            ts = None if self._values_only else copy_of(result.timestamps, n, np.int64)
            values = copy_of(result.values, n, np.float32)
            rows = copy_of(result.rows_per_segment, n_segments, np.uint32)
            tags = [copy_of(context.lib.mdb_grid_result_tag_views(out, t), n, np.uint8, 16)
                    for t in range(self._n_tags)]
            return ts, values, rows, result.metrics.as_dict(), tags
        finally:
            context.lib.mdb_grid_result_free(out)

    def cancel(self):
        if self._pointer is not None:
            self._context.lib.mdb_grid_cancel(self._pointer)
            self._pointer = None

    def __del__(self):
        try:
            self.cancel()
        except Exception:
            pass


def comm_unique_id():
    """ncclGetUniqueId through the C ABI: 128 bytes, made by one rank."""
    lib = _abi.load_hip_library()
    buffer = C.create_string_buffer(_abi.MDB_COMM_ID_BYTES)
    if lib.mdb_comm_unique_id(buffer) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return buffer.raw


# mdb_agg_state as a numpy record: the cells of mdb_agg_buckets*, row-major [n_groups][n_buckets].
AGG_STATE_DTYPE = np.dtype([("sum", "<f8"), ("count", "<i8"), ("min", "<f4"), ("max", "<f4")])
assert AGG_STATE_DTYPE.itemsize == C.sizeof(_abi.AggStateC)

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def fresh_agg_states(shape):
    """Fresh states {0, 0, FLT_MAX, -FLT_MAX} (f32::MAX / f32::MIN, model_simple_aggregates.rs:413, 456)."""
    states = np.zeros(shape, dtype=AGG_STATE_DTYPE)
    states["min"] = _abi.F32_MAX
    states["max"] = -_abi.F32_MAX
    return states


def agg_merge_n(into, other):
    """into[k] = merge(into[k], other[k]) in place (mdb_agg_merge_n): two arrays of AGG_STATE_DTYPE of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != AGG_STATE_DTYPE or other.dtype != AGG_STATE_DTYPE or into.size != other.size:
        raise ValueError("agg_merge_n takes two state arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("agg_merge_n merges into a contiguous array")
    other = np.ascontiguousarray(other)
    if lib.mdb_agg_merge_n(into.ctypes.data_as(C.c_void_p), other.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


# mdb_m4_cell as a numpy record: the cells of mdb_m4_buckets*, row-major [n_groups][n_buckets].
M4_CELL_DTYPE = np.dtype([("count", "<i8"), ("t_first", "<i8"), ("t_last", "<i8"), ("t_min", "<i8"), ("t_max", "<i8"),
                          ("v_first", "<f4"), ("v_last", "<f4"), ("v_min", "<f4"), ("v_max", "<f4")])
assert M4_CELL_DTYPE.itemsize == C.sizeof(_abi.M4CellC)


def fresh_m4_cells(shape):
    """Fresh (empty) M4 cells: all-zero bytes."""
    return np.zeros(shape, dtype=M4_CELL_DTYPE)


def m4_merge(into, from_):
    """into[k] merged with from_[k] in place by the four rules of mdb_m4_buckets (mdb_m4_merge_n): two arrays of
    M4_CELL_DTYPE of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != M4_CELL_DTYPE or from_.dtype != M4_CELL_DTYPE or into.size != from_.size:
        raise ValueError("m4_merge takes two cell arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("m4_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_m4_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


# mdb_moments_cell as a numpy record: the cells of mdb_moments_buckets*, row-major [n_groups][n_buckets].
MOMENTS_CELL_DTYPE = np.dtype([("count", "<i8"), ("mean", "<f8"), ("m2", "<f8")])
assert MOMENTS_CELL_DTYPE.itemsize == C.sizeof(_abi.MomentsCellC)


def fresh_moments_cells(shape):
    """Fresh (empty) moments cells: all-zero bytes."""
    return np.zeros(shape, dtype=MOMENTS_CELL_DTYPE)


def moments_merge(into, from_):
    """into[k] merged with from_[k] in place by the merge rule of mdb_moments_buckets (mdb_moments_merge_n): two
    arrays of MOMENTS_CELL_DTYPE of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != MOMENTS_CELL_DTYPE or from_.dtype != MOMENTS_CELL_DTYPE or into.size != from_.size:
        raise ValueError("moments_merge takes two cell arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("moments_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_moments_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


def moments_variance(cells, ddof=1):
    """m2 / (count - ddof) per cell (mdb_moments_variance): ddof 0 is var_pop, 1 var_samp; NaN where the count does not
    allow it. The standard deviation is its np.sqrt. Returns float64 of the shape of `cells`."""
    lib = _abi.load_hip_library()
    if cells.dtype != MOMENTS_CELL_DTYPE:
        raise ValueError("moments_variance takes an array of MOMENTS_CELL_DTYPE")
    if ddof < 0:
        raise ValueError("ddof must be 0 or 1")
    flat = np.ascontiguousarray(cells).reshape(-1)
    out = np.empty(flat.size, dtype=np.float64)
    if lib.mdb_moments_variance(flat.ctypes.data_as(C.c_void_p), flat.size, int(ddof),
                                out.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out.reshape(cells.shape)


# mdb_comoments_cell as a numpy record: the cells of mdb_comoments_buckets*, row-major [n_groups][n_buckets].
COMOMENTS_CELL_DTYPE = np.dtype([("count", "<i8"), ("mean_x", "<f8"), ("mean_y", "<f8"), ("m2_x", "<f8"),
                                 ("m2_y", "<f8"), ("c_xy", "<f8")])
assert COMOMENTS_CELL_DTYPE.itemsize == C.sizeof(_abi.ComomentsCellC)

# The statistics of mdb_comoments_finish (MDB_COMOMENTS_*); x is the independent variable: SQL's regr_*(y, x).
COMOMENTS_KINDS = {"covar_pop": 0, "covar_samp": 1, "corr": 2, "regr_slope": 3, "regr_intercept": 4, "regr_r2": 5}


def fresh_comoments_cells(shape):
    """Fresh (empty) comoments cells: all-zero bytes."""
    return np.zeros(shape, dtype=COMOMENTS_CELL_DTYPE)


def comoments_merge(into, from_):
    """into[k] merged with from_[k] in place by the merge rule of mdb_comoments_buckets (mdb_comoments_merge_n): two
    arrays of COMOMENTS_CELL_DTYPE of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != COMOMENTS_CELL_DTYPE or from_.dtype != COMOMENTS_CELL_DTYPE or into.size != from_.size:
        raise ValueError("comoments_merge takes two cell arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("comoments_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_comoments_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


def comoments_moments(cells, which):
    """The (count, mean, m2) of field `which` (0 or "x", 1 or "y") of every cell as MOMENTS_CELL_DTYPE
    (mdb_comoments_moments): what moments_variance takes."""
    lib = _abi.load_hip_library()
    if cells.dtype != COMOMENTS_CELL_DTYPE:
        raise ValueError("comoments_moments takes an array of COMOMENTS_CELL_DTYPE")
    which = {"x": 0, "y": 1}.get(which, which)
    flat = np.ascontiguousarray(cells).reshape(-1)
    out = fresh_moments_cells(flat.size)
    if lib.mdb_comoments_moments(flat.ctypes.data_as(C.c_void_p), flat.size, int(which),
                                 out.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out.reshape(cells.shape)


def comoments_finish(cells, kind):
    """The statistic `kind` (a name of COMOMENTS_KINDS or its number) per cell (mdb_comoments_finish): covar_pop,
    covar_samp, corr, regr_slope, regr_intercept, regr_r2 - the regr_* with x as the independent variable; NaN where
    the cell does not allow it. Returns float64 of the shape of `cells`."""
    lib = _abi.load_hip_library()
    if cells.dtype != COMOMENTS_CELL_DTYPE:
        raise ValueError("comoments_finish takes an array of COMOMENTS_CELL_DTYPE")
    kind = COMOMENTS_KINDS.get(kind, kind)
    flat = np.ascontiguousarray(cells).reshape(-1)
    out = np.empty(flat.size, dtype=np.float64)
    if lib.mdb_comoments_finish(flat.ctypes.data_as(C.c_void_p), flat.size, int(kind),
                                out.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out.reshape(cells.shape)


# mdb_derived_cell as a numpy record: the cells of mdb_derived_buckets*, row-major [n_groups][n_buckets].
DERIVED_CELL_DTYPE = np.dtype([("count", "<i8"), ("mean", "<f8"), ("m2", "<f8"), ("min", "<f4"), ("max", "<f4")])
assert DERIVED_CELL_DTYPE.itemsize == C.sizeof(_abi.DerivedCellC) == 32

# The operations of mdb_derived_expr (MDB_DERIVED_*): z = ((a * x) + (b * y)) + c, (a * (x * y)) + c, (a * (x / y)) + c.
DERIVED_OPS = {"linear": 0, "product": 1, "ratio": 2}


def derived_expr(op, a=1.0, b=1.0, c=0.0, absolute=False):
    """An mdb_derived_expr: `op` a name of DERIVED_OPS or its number; `absolute` sets MDB_DERIVED_ABS. An expression
    made elsewhere (a DerivedExprC) is returned as it is."""
    if isinstance(op, _abi.DerivedExprC):
        return op
    return _abi.DerivedExprC(int(DERIVED_OPS.get(op, op)), _abi.MDB_DERIVED_ABS if absolute else 0, a, b, c)


def fresh_derived_cells(shape):
    """Fresh (empty) derived cells: all-zero bytes."""
    return np.zeros(shape, dtype=DERIVED_CELL_DTYPE)


def derived_apply(expr, x, y):
    """z = f(x, y) element for element on the host (mdb_derived_apply): the evaluator the kernels use, binary32
    operations in the written order. x and y: float32 arrays of one size; returns float32 of the shape of x."""
    lib = _abi.load_hip_library()
    x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    if x.size != y.size:
        raise ValueError("derived_apply takes two arrays of one size")
    z = np.empty(x.shape, dtype=np.float32)
    expr = derived_expr(expr)
    if lib.mdb_derived_apply(C.byref(expr), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size,
                             z.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return z


def derived_merge(into, from_):
    """into[k] merged with from_[k] in place by the merge rule of mdb_derived_buckets (mdb_derived_merge_n): two arrays
    of DERIVED_CELL_DTYPE of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != DERIVED_CELL_DTYPE or from_.dtype != DERIVED_CELL_DTYPE or into.size != from_.size:
        raise ValueError("derived_merge takes two cell arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("derived_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_derived_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


def derived_stats(cells):
    """(count, mean, m2) per cell as an array of MOMENTS_CELL_DTYPE (mdb_derived_stats): what moments_variance takes."""
    lib = _abi.load_hip_library()
    if cells.dtype != DERIVED_CELL_DTYPE:
        raise ValueError("derived_stats takes an array of DERIVED_CELL_DTYPE")
    flat = np.ascontiguousarray(cells).reshape(-1)
    out = np.zeros(flat.size, dtype=MOMENTS_CELL_DTYPE)
    if lib.mdb_derived_stats(flat.ctypes.data_as(C.c_void_p), flat.size, out.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out.reshape(cells.shape)


EPISODE_DTYPE = np.dtype([("first_row", "<u8"), ("count", "<u8"), ("t_first", "<i8"), ("t_last", "<i8"), ("sum", "<f8"),
                          ("min", "<f4"), ("max", "<f4"), ("group", "<u4"), ("first_segment", "<u4"), ("reserved", "<u8")])
assert EPISODE_DTYPE.itemsize == C.sizeof(_abi.EpisodeC) == 64

# mdb_integral_cell as a numpy record: the cells of mdb_integral_buckets*, row-major [n_groups][n_buckets].
INTEGRAL_CELL_DTYPE = np.dtype([("duration", "<u8"), ("integral", "<f8")])
assert INTEGRAL_CELL_DTYPE.itemsize == C.sizeof(_abi.IntegralCellC) == 16
MDB_INTEGRAL_LINEAR = _abi.MDB_INTEGRAL_LINEAR
MDB_INTEGRAL_STEP = _abi.MDB_INTEGRAL_STEP


def fresh_integral_cells(shape):
    """Fresh (empty) integral cells: all-zero bytes."""
    return np.zeros(shape, dtype=INTEGRAL_CELL_DTYPE)


def integral_merge(into, from_):
    """into[k] += from_[k] in place, both members (mdb_integral_merge_n): two arrays of INTEGRAL_CELL_DTYPE of one
    size."""
    lib = _abi.load_hip_library()
    if into.dtype != INTEGRAL_CELL_DTYPE or from_.dtype != INTEGRAL_CELL_DTYPE or into.size != from_.size:
        raise ValueError("integral_merge takes two cell arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("integral_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_integral_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


def integral_average(cells):
    """The time-weighted average integral / duration per cell (mdb_integral_average), NaN where duration == 0.
    Returns float64 of the shape of `cells`."""
    lib = _abi.load_hip_library()
    if cells.dtype != INTEGRAL_CELL_DTYPE:
        raise ValueError("integral_average takes an array of INTEGRAL_CELL_DTYPE")
    flat = np.ascontiguousarray(cells).reshape(-1)
    out = np.empty(flat.size, dtype=np.float64)
    if lib.mdb_integral_average(flat.ctypes.data_as(C.c_void_p), flat.size, out.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out.reshape(cells.shape)



# mdb_sample_cell as a numpy record: the cells of mdb_sample_at*, row-major [n_groups][n_instants].
SAMPLE_CELL_DTYPE = np.dtype([("count", "<u8"), ("sum", "<f8")])
assert SAMPLE_CELL_DTYPE.itemsize == C.sizeof(_abi.SampleCellC) == 16
MDB_SAMPLE_LINEAR = _abi.MDB_SAMPLE_LINEAR
MDB_SAMPLE_STEP = _abi.MDB_SAMPLE_STEP
MDB_SAMPLE_EXACT = _abi.MDB_SAMPLE_EXACT


def fresh_sample_cells(shape):
    """Fresh (empty) sample cells: all-zero bytes."""
    return np.zeros(shape, dtype=SAMPLE_CELL_DTYPE)


def sample_merge(into, from_):
    """into[k] merged with from_[k] in place (mdb_sample_merge_n): a cell with count == 0 takes the other whole, else
    both members are added. Two arrays of SAMPLE_CELL_DTYPE of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != SAMPLE_CELL_DTYPE or from_.dtype != SAMPLE_CELL_DTYPE or into.size != from_.size:
        raise ValueError("sample_merge takes two cell arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("sample_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_sample_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


def sample_values(cells):
    """The sampled value sum / count per cell (mdb_sample_values), NaN where count == 0: the gaps of gap-fill.
    Returns float64 of the shape of `cells`."""
    lib = _abi.load_hip_library()
    if cells.dtype != SAMPLE_CELL_DTYPE:
        raise ValueError("sample_values takes an array of SAMPLE_CELL_DTYPE")
    flat = np.ascontiguousarray(cells).reshape(-1)
    out = np.empty(flat.size, dtype=np.float64)
    if lib.mdb_sample_values(flat.ctypes.data_as(C.c_void_p), flat.size, out.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out.reshape(cells.shape)


# mdb_change_cell as a numpy record: the cells of mdb_change_buckets*, row-major [n_groups][n_buckets].
CHANGE_CELL_DTYPE = np.dtype([("count", "<u8"), ("n_fall", "<u8"), ("duration", "<u8"), ("rise", "<f8"), ("fall", "<f8"),
                              ("reset_sum", "<f8"), ("max_rise", "<f8"), ("max_fall", "<f8")])
assert CHANGE_CELL_DTYPE.itemsize == C.sizeof(_abi.ChangeCellC) == 64
MDB_CHANGE_NET = _abi.MDB_CHANGE_NET
MDB_CHANGE_VARIATION = _abi.MDB_CHANGE_VARIATION
MDB_CHANGE_INCREASE = _abi.MDB_CHANGE_INCREASE
MDB_CHANGE_RATE = _abi.MDB_CHANGE_RATE


def fresh_change_cells(shape):
    """Fresh (empty) change cells: all-zero bytes."""
    return np.zeros(shape, dtype=CHANGE_CELL_DTYPE)


def change_merge(into, from_):
    """into[k] merged with from_[k] in place (mdb_change_merge_n): the integers and the sums added, the larger of each
    maximum. Two arrays of CHANGE_CELL_DTYPE of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != CHANGE_CELL_DTYPE or from_.dtype != CHANGE_CELL_DTYPE or into.size != from_.size:
        raise ValueError("change_merge takes two cell arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("change_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_change_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


def change_finish(cells, kind):
    """One figure per cell (mdb_change_finish): MDB_CHANGE_NET rise - fall, MDB_CHANGE_VARIATION rise + fall,
    MDB_CHANGE_INCREASE rise + reset_sum, MDB_CHANGE_RATE the increase per second; NaN where count == 0 (RATE: or
    duration == 0). Returns float64 of the shape of `cells`."""
    lib = _abi.load_hip_library()
    if cells.dtype != CHANGE_CELL_DTYPE:
        raise ValueError("change_finish takes an array of CHANGE_CELL_DTYPE")
    flat = np.ascontiguousarray(cells).reshape(-1)
    out = np.empty(flat.size, dtype=np.float64)
    if lib.mdb_change_finish(flat.ctypes.data_as(C.c_void_p), flat.size, int(kind), out.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out.reshape(cells.shape)


# The kinds of mdb_roll_request (MDB_ROLL_*) and the numpy type of their cells: the cell type names the merge rule.
MDB_ROLL_AGG, MDB_ROLL_M4, MDB_ROLL_MOMENTS, MDB_ROLL_COMOMENTS = (_abi.MDB_ROLL_AGG, _abi.MDB_ROLL_M4, _abi.MDB_ROLL_MOMENTS,
                                                                  _abi.MDB_ROLL_COMOMENTS)
MDB_ROLL_DERIVED, MDB_ROLL_INTEGRAL, MDB_ROLL_CHANGE, MDB_ROLL_U64 = (_abi.MDB_ROLL_DERIVED, _abi.MDB_ROLL_INTEGRAL,
                                                                      _abi.MDB_ROLL_CHANGE, _abi.MDB_ROLL_U64)
ROLL_KINDS = {
    MDB_ROLL_AGG: AGG_STATE_DTYPE,              # agg_buckets*
    MDB_ROLL_M4: M4_CELL_DTYPE,                 # m4_buckets*
    MDB_ROLL_MOMENTS: MOMENTS_CELL_DTYPE,       # moments_buckets*, binned_buckets*
    MDB_ROLL_COMOMENTS: COMOMENTS_CELL_DTYPE,   # comoments_buckets*, trend_buckets*
    MDB_ROLL_DERIVED: DERIVED_CELL_DTYPE,       # derived_buckets*
    MDB_ROLL_INTEGRAL: INTEGRAL_CELL_DTYPE,     # integral_buckets*
    MDB_ROLL_CHANGE: CHANGE_CELL_DTYPE,         # change_buckets*
    MDB_ROLL_U64: np.dtype("<u8"),              # hist_buckets*, dwell_buckets*, transit_buckets*: wrapping add
}


def roll_windows(n_buckets, window, stride=1):
    """The number of whole windows of `window` buckets every `stride` buckets in `n_buckets` buckets
    (mdb_roll_windows): 0 when n_buckets < window, else (n_buckets - window) // stride + 1."""
    lib = _abi.load_hip_library()
    request = _abi.RollRequestC(MDB_ROLL_U64, 0, 1, int(n_buckets), 1, int(window), int(stride))
    n_windows = C.c_uint64()
    if lib.mdb_roll_windows(C.byref(request), C.byref(n_windows)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return n_windows.value


def roll_kind_of(dtype):
    """The MDB_ROLL_* kind whose cells have the numpy type `dtype`."""
    for kind, cell_dtype in ROLL_KINDS.items():
        if dtype == cell_dtype:
            return kind
    raise ValueError(f"no MDB_ROLL_* kind has cells of type {dtype}: see ROLL_KINDS (sample cells do not roll)")


def roll_cells(cells, window, stride=1, kind=None):
    """Rolling windows over the cells of a per-bucket operator, on the host (mdb_roll_cells): axis 1 of `cells` is the
    bucket axis, the axes behind it are taken as one (n_inner), a 1-D array is one column. Window k is the merge of
    the buckets [k * stride, k * stride + window) by the operator's own merge rule in the fixed order mdb.h states,
    so Context.roll_cells_dev gives the same bytes. `kind` (MDB_ROLL_*) defaults to the one of the array's type.
    Returns the windows with axis 1 of length roll_windows(n_buckets, window, stride)."""
    lib = _abi.load_hip_library()
    cells = np.ascontiguousarray(cells)
    kind = roll_kind_of(cells.dtype) if kind is None else int(kind)
    if kind in ROLL_KINDS and cells.dtype != ROLL_KINDS[kind]:
        raise ValueError(f"kind {kind} rolls cells of type {ROLL_KINDS[kind]}")
    if cells.ndim == 0:
        raise ValueError("roll_cells takes an array with a bucket axis")
    shape = (1, cells.shape[0]) if cells.ndim == 1 else cells.shape
    n_outer, n_buckets = shape[0], shape[1]
    n_inner = int(np.prod(shape[2:], dtype=np.int64))
    request = _abi.RollRequestC(kind, 0, n_outer, n_buckets, n_inner, int(window), int(stride))
    n_windows = C.c_uint64()
    if lib.mdb_roll_windows(C.byref(request), C.byref(n_windows)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    out_shape = (n_windows.value,) if cells.ndim == 1 else (n_outer, n_windows.value) + tuple(shape[2:])
    out = np.zeros(out_shape, dtype=cells.dtype)
    if lib.mdb_roll_cells(C.byref(request), cells.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out


def _f64_key(x):
    """IEEE 754 totalOrder key of an f64 bit pattern (signed integer comparison)."""
    bits = struct.unpack("<q", struct.pack("<d", x))[0]
    return bits ^ ((bits >> 63) & 0x7FFFFFFFFFFFFFFF)


def _f32_bits_of_key(key):
    return (key ^ ((key >> 31) & 0x7FFFFFFF)) & 0xFFFFFFFF


def _f64_key_of_f32(key):
    """The f64 totalOrder key of the f32 with totalOrder key `key` (f32 -> f64 is exact and keeps the order, NaN
    payloads included: they move up by 29 bits)."""
    bits = _f32_bits_of_key(key)
    if (bits >> 23) & 0xFF == 0xFF and bits & 0x7FFFFF:
        wide = ((bits >> 31) << 63) | (0x7FF << 52) | ((bits & 0x7FFFFF) << 29)
        wide -= 1 << 64 if wide >> 63 else 0
        return wide ^ ((wide >> 63) & 0x7FFFFFFFFFFFFFFF)
    return _f64_key(struct.unpack("<f", struct.pack("<I", bits))[0])


def _first_f32_key(passes):
    """The smallest f32 totalOrder key for which passes(f64 key of that f32) holds (monotone false..true), or None."""
    lo, hi = -(1 << 31), (1 << 31) - 1
    if not passes(_f64_key_of_f32(hi)):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if passes(_f64_key_of_f32(mid)):
            hi = mid
        else:
            lo = mid + 1
    return lo


def value_filter(lo=None, hi=None, lo_open=False, hi_open=False, t_lo=None, t_hi=None):
    """An mdb_value_filter for `lo <(=) value <(=) hi AND t_lo <= ts <= t_hi` (None: no bound). lo and hi are Python
    floats (f64); they are converted exactly, so the filter selects exactly the f32 values v for which float(v) op
    literal holds in f64 IEEE totalOrder (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN) - the order of arrow's
    float comparison kernels. The f32 bounds are closed, written by bit pattern (NaN payloads included)."""
    flags, lo_bits, hi_bits = 0, 0, 0
    empty = False
    if lo is None:
        flags |= _abi.MDB_VALUE_NO_LO
    else:
        bound = _f64_key(float(lo))
        key = _first_f32_key((lambda k: k > bound) if lo_open else (lambda k: k >= bound))
        if key is None:
            empty = True
        else:
            lo_bits = _f32_bits_of_key(key)
    if hi is None:
        flags |= _abi.MDB_VALUE_NO_HI
    else:
        bound = _f64_key(float(hi))
        # the largest key that passes is one below the smallest that fails
        key = _first_f32_key((lambda k: k >= bound) if hi_open else (lambda k: k > bound))
        if key == -(1 << 31):
            empty = True
        else:
            hi_bits = _f32_bits_of_key((1 << 31) - 1 if key is None else key - 1)
    if empty:  # no f32 value passes: (+NaN with the largest payload, ...) is empty
        flags = _abi.MDB_VALUE_LO_OPEN | _abi.MDB_VALUE_NO_HI
        lo_bits = 0x7FFFFFFF
    result = _abi.ValueFilterC(INT64_MIN if t_lo is None else int(t_lo), INT64_MAX if t_hi is None else int(t_hi),
                               0.0, 0.0, flags, 0)
    for field, bits in (("v_lo", lo_bits), ("v_hi", hi_bits)):
        C.memmove(C.addressof(result) + getattr(_abi.ValueFilterC, field).offset, C.byref(C.c_uint32(bits)), 4)
    return result


def value_filter_bits(flt):
    """(v_lo bits, v_hi bits) of an mdb_value_filter, as uint32 (the f32 fields read without a float conversion)."""
    raw = C.string_at(C.addressof(flt), C.sizeof(flt))
    return struct.unpack_from("<I", raw, _abi.ValueFilterC.v_lo.offset)[0], \
        struct.unpack_from("<I", raw, _abi.ValueFilterC.v_hi.offset)[0]


def unpack_mask(raw, n_rows):
    """The bytes of a row mask (little-endian words: an Arrow boolean bitmap) as a bool array of n_rows entries."""
    raw = np.ascontiguousarray(raw).view(np.uint8)
    return np.unpackbits(raw, bitorder="little")[: int(n_rows)].astype(bool)


def mask_words(n_rows):
    """64-bit words of a row mask over n_rows rows (mdb.h: row r is bit r % 64 of word r / 64)."""
    return (int(n_rows) + 63) // 64


def is_value_within_error_bound(eb, real_value, approximate_value):
    """models/mod.rs:53-77 through the C ABI (host arithmetic, no GPU)."""
    lib = _abi.load_hip_library()
    within = C.c_int32()
    if lib.mdb_is_value_within_error_bound(eb, real_value, approximate_value, C.byref(within)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return bool(within.value)


def are_compressed_timestamps_regular(data):
    """models/timestamps.rs:199-202 through the C ABI (host arithmetic, no GPU)."""
    lib = _abi.load_hip_library()
    data = bytes(data)
    regular = C.c_int32()
    if lib.mdb_are_compressed_timestamps_regular(data, len(data), C.byref(regular)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return bool(regular.value)


MDB_DWELL_STEP = _abi.MDB_DWELL_STEP


def dwell_merge(into, from_):
    """into[k] += from_[k] in place (mdb_dwell_merge_n): two uint64 arrays of dwell_buckets of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != np.uint64 or from_.dtype != np.uint64 or into.size != from_.size:
        raise ValueError("dwell_merge takes two uint64 arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("dwell_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_dwell_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


def dwell_share(dwell):
    """The share of its (group, bucket) row's linked time each cell holds (mdb_dwell_share): dwell / the sum over the
    last axis, NaN where that sum is 0. Returns float64 of the shape of `dwell`."""
    lib = _abi.load_hip_library()
    if dwell.dtype != np.uint64 or dwell.ndim < 1:
        raise ValueError("dwell_share takes a uint64 array whose last axis is the cells")
    n_cells = dwell.shape[-1]
    flat = np.ascontiguousarray(dwell).reshape(-1)
    out = np.empty(flat.size, dtype=np.float64)
    if n_cells and lib.mdb_dwell_share(flat.ctypes.data_as(C.c_void_p), flat.size // n_cells, n_cells,
                                       out.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return out.reshape(dwell.shape)


def transit_merge(into, from_):
    """into[k] += from_[k] in place (mdb_transit_merge_n): two uint64 arrays of transit_buckets of one size."""
    lib = _abi.load_hip_library()
    if into.dtype != np.uint64 or from_.dtype != np.uint64 or into.size != from_.size:
        raise ValueError("transit_merge takes two uint64 arrays of one size")
    if not into.flags.c_contiguous:
        raise ValueError("transit_merge merges into a contiguous array")
    from_ = np.ascontiguousarray(from_)
    if lib.mdb_transit_merge_n(into.ctypes.data_as(C.c_void_p), from_.ctypes.data_as(C.c_void_p), into.size) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return into


def transit_crossings(counts):
    """The pairs that went over each edge (mdb_transit_crossings): `counts` is uint64 (..., n_cells, n_cells), indexed
    [from][to]; returns (up, down), uint64 of shape (..., n_cells - 1): up[..., e] is the sum of counts[from <= e < to],
    down[..., e] the sum of counts[to <= e < from]."""
    lib = _abi.load_hip_library()
    if counts.dtype != np.uint64 or counts.ndim < 2 or counts.shape[-1] != counts.shape[-2] or counts.shape[-1] < 1:
        raise ValueError("transit_crossings takes a uint64 array whose last two axes are the cells [from][to]")
    n_cells = counts.shape[-1]
    flat = np.ascontiguousarray(counts).reshape(-1)
    n_rows = flat.size // (n_cells * n_cells)
    up = np.zeros(n_rows * (n_cells - 1), dtype=np.uint64)
    down = np.zeros(n_rows * (n_cells - 1), dtype=np.uint64)
    if lib.mdb_transit_crossings(flat.ctypes.data_as(C.c_void_p), n_rows, n_cells, up.ctypes.data_as(C.c_void_p),
                                 down.ctypes.data_as(C.c_void_p)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    shape = counts.shape[:-2] + (n_cells - 1,)
    return up.reshape(shape), down.reshape(shape)


def _edges_array(edges):
    edges = np.ascontiguousarray(edges, dtype=np.float32)
    if edges.ndim != 1:
        raise ValueError("edges must be a one-dimensional array of float32")
    return edges


def hist_cell_of(edges, value):
    """The cell of `value` under `edges` (mdb_hist_cell_of: the number of edges at or below it in totalOrder; host
    arithmetic, no GPU). Raises for edges mdb_hist_batch would reject."""
    lib = _abi.load_hip_library()
    edges = _edges_array(edges)
    cell = C.c_uint32()
    value = C.c_float.from_buffer_copy(np.asarray(value, dtype=np.float32).tobytes())  # (keeps a NaN's payload)
    if lib.mdb_hist_cell_of(edges.ctypes.data_as(C.c_void_p), len(edges), value, C.byref(cell)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return cell.value


def quantile_positions(q, n_points):
    """(rank_lo, rank_hi, fraction) of quantile q over n_points points (mdb_quantile_positions; host arithmetic)."""
    lib = _abi.load_hip_library()
    rank_lo, rank_hi, fraction = C.c_uint64(), C.c_uint64(), C.c_double()
    if lib.mdb_quantile_positions(float(q), int(n_points), C.byref(rank_lo), C.byref(rank_hi), C.byref(fraction)) != 0:
        raise HipError(lib.mdb_last_error().decode())
    return rank_lo.value, rank_hi.value, fraction.value


class Context:
    def __init__(self, device=0):
        self.lib = _abi.load_hip_library()
        self.handle = C.c_void_p()
        if self.lib.mdb_init(int(device), C.byref(self.handle)) != 0:
            raise HipError(self.lib.mdb_last_error().decode())
        self.device = device
        self.last_call_seconds = 0.0

    def _check(self, code):
        if code != 0:
            raise HipError(self.lib.mdb_last_error().decode())

    def close(self):
        if self.handle:
            self.lib.mdb_close(self.handle)
            self.handle = C.c_void_p()

    def clone(self):
        """Another context on the same device (mdb_clone): its own stream and scratch."""
        other = Context.__new__(Context)
        other.lib, other.device, other.handle = self.lib, self.device, C.c_void_p()
        self._check(self.lib.mdb_clone(self.handle, C.byref(other.handle)))
        return other

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, hbm = C.c_int32(), C.c_uint64()
        self._check(self.lib.mdb_device_info(self.handle, name, 256, C.byref(cus), C.byref(hbm)))
        return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}

    def set_stream(self, hip_stream):
        self._check(self.lib.mdb_set_stream(self.handle, C.c_void_p(hip_stream)))

    def trim(self):
        """Give back the scratch / staging memory the context has grown; returns the device bytes."""
        released = C.c_uint64()
        self._check(self.lib.mdb_trim(self.handle, C.byref(released)))
        return released.value

    def set_scratch_limit(self, nbytes):
        """Device scratch beyond `nbytes` is given back after every call (0: keep everything). Refused for it are the
        calls whose one array alone is larger: the value columns of comoments_buckets* and derived_* (4 B per row each)
        and the suffix folds of roll_cells_dev (at most the bytes of its cells)."""
        self._check(self.lib.mdb_set_scratch_limit(self.handle, C.c_uint64(nbytes)))

    # ---- device memory -----------------------------------------------------------------------

    def dev_alloc(self, nbytes):
        pointer = C.c_void_p()
        self._check(self.lib.mdb_dev_alloc(self.handle, int(nbytes), C.byref(pointer)))
        return pointer.value

    def dev_free(self, pointer):
        self._check(self.lib.mdb_dev_free(self.handle, C.c_void_p(pointer)))

    def upload_array(self, array):
        array = np.ascontiguousarray(array)
        pointer = self.dev_alloc(max(array.nbytes, 1))
        self._check(self.lib.mdb_dev_upload(self.handle, C.c_void_p(pointer),
                                            array.ctypes.data_as(C.c_void_p), array.nbytes))
        return pointer

    def download_array(self, pointer, count, dtype, offset_elements=0):
        out = np.empty(count, dtype=dtype)
        source = pointer + offset_elements * out.itemsize
        self._check(self.lib.mdb_dev_download(self.handle, out.ctypes.data_as(C.c_void_p),
                                              C.c_void_p(source), out.nbytes))
        return out

    def sync(self):
        self._check(self.lib.mdb_dev_sync(self.handle))

    def upload_segments(self, batch):
        seg = batch.as_c()
        out = C.POINTER(_abi.SegmentsOwnedC)()
        self._check(self.lib.mdb_segments_upload(self.handle, C.byref(seg), C.byref(out)))
        return DeviceSegments(self, out)

    # ---- grid ------------------------------------------------------------------------------------

    def grid_count(self, batch):
        seg = batch.as_c()
        n_out = C.c_uint64()
        self._check(self.lib.mdb_grid_count(self.handle, C.byref(seg), C.byref(n_out)))
        return n_out.value

    def grid_batch(self, batch, cap=None):
        """Returns (timestamps i64[], values f32[], rows_per_segment u32[], metrics dict)."""
        seg = batch.as_c()
        if cap is None:
            cap = self.grid_count(batch)
        out_ts = np.empty(cap, dtype=np.int64)
        out_val = np.empty(cap, dtype=np.float32)
        rows = np.empty(len(batch), dtype=np.uint32)
        n_out = C.c_uint64()
        metrics = _abi.GridMetricsC()
        self._check(self.lib.mdb_grid_batch(
            self.handle, C.byref(seg), out_ts.ctypes.data_as(C.c_void_p),
            out_val.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), cap,
            C.byref(n_out), C.byref(metrics)))
        return out_ts[: n_out.value], out_val[: n_out.value], rows, metrics.as_dict()

    def grid_batch_owned(self, batch, time_range=None, copy=True, values_only=False):
        """One-call grid into page-locked memory owned by the library (mdb_grid_batch_owned).
        Returns (timestamps, values, rows_per_segment, metrics); the arrays are copies unless
        copy=False, in which case they alias the library's buffer and `release()` (5th item) must
        be called when done. values_only=True skips the timestamps (None is returned for them)."""
        seg = batch.as_c()
        out = C.POINTER(_abi.GridResultC)()
        has_range = time_range is not None
        t_lo, t_hi = time_range if has_range else (0, 0)
        flags = (1 if has_range else 0) | (2 if values_only else 0)
        self._check(self.lib.mdb_grid_batch_owned(self.handle, C.byref(seg), flags, t_lo, t_hi, 0,
                                                  C.byref(out)))
        result = out.contents
        n, n_segments = int(result.n), int(result.n_segments)

        def view(pointer, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            buffer = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(pointer)
            return np.frombuffer(buffer, dtype=dtype)

        ts = None if values_only else view(result.timestamps, n, np.int64)
        values = view(result.values, n, np.float32)
        rows = view(result.rows_per_segment, n_segments, np.uint32)
        metrics = result.metrics.as_dict()
        release = lambda: self.lib.mdb_grid_result_free(out)
        if copy:
            ts = None if ts is None else ts.copy()
            values, rows = values.copy(), rows.copy()
            release()
            return ts, values, rows, metrics
        return ts, values, rows, metrics, release

    def grid_submit(self, batches, tag_views=None, tag_buffer_shifts=None, time_range=None,
                    values_only=False, reserve_front=0):
        """mdb_grid_submit: one or several SegmentBatches through one launch, on a worker thread of the
        library. tag_views: per batch, a list of (n, 16)-byte uint8 arrays (one per tag column) with one
        view per segment; tag_buffer_shifts: per batch, one int per tag column. Returns a GridTicket."""
        batches = list(batches)
        n_tags = len(tag_views[0]) if tag_views else 0
        inputs = (_abi.GridInputC * len(batches))()
        keep = [batches]
        for b, batch in enumerate(batches):
            inputs[b].segments = batch.as_c()
            if n_tags:
                views = [np.ascontiguousarray(v, dtype=np.uint8) for v in tag_views[b]]
                pointers = (C.c_void_p * n_tags)(*[v.ctypes.data for v in views])
                shifts = (C.c_int32 * n_tags)(*(tag_buffer_shifts[b] if tag_buffer_shifts else [0] * n_tags))
                inputs[b].tag_views = pointers
                inputs[b].tag_buffer_shift = shifts
                keep += [views, pointers, shifts]
        has_range = time_range is not None
        t_lo, t_hi = time_range if has_range else (0, 0)
        request = _abi.GridRequestC((1 if has_range else 0) | (2 if values_only else 0), n_tags, t_lo, t_hi,
                                    reserve_front)
        ticket = C.c_void_p()
        self._check(self.lib.mdb_grid_submit(self.handle, inputs, len(batches), C.byref(request),
                                             C.byref(ticket)))
        return GridTicket(self, ticket, keep, n_tags, values_only)

    def replicate_views(self, views, rows_per_segment, buffer_shift=0):
        """mdb_replicate_views: views (n, 16) uint8 -> (sum(rows), 16) uint8."""
        views = np.ascontiguousarray(views, dtype=np.uint8).reshape(-1, 16)
        rows = np.ascontiguousarray(rows_per_segment, dtype=np.uint32)
        out = np.empty((int(rows.sum()), 16), dtype=np.uint8)
        self._check(self.lib.mdb_replicate_views(views.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                                 len(rows), buffer_shift, out.ctypes.data_as(C.c_void_p), len(out)))
        return out

    def grid_batch_range(self, batch, t_lo, t_hi):
        """grid() with the predicate t_lo <= timestamp <= t_hi pushed down."""
        seg = batch.as_c()
        n_out = C.c_uint64()
        self._check(self.lib.mdb_grid_count_range(self.handle, C.byref(seg), t_lo, t_hi,
                                                  C.byref(n_out)))
        cap = n_out.value
        out_ts = np.empty(cap, dtype=np.int64)
        out_val = np.empty(cap, dtype=np.float32)
        rows = np.empty(len(batch), dtype=np.uint32)
        metrics = _abi.GridMetricsC()
        self._check(self.lib.mdb_grid_batch_range(
            self.handle, C.byref(seg), t_lo, t_hi, out_ts.ctypes.data_as(C.c_void_p),
            out_val.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), cap,
            C.byref(n_out), C.byref(metrics)))
        return out_ts[: n_out.value], out_val[: n_out.value], rows, metrics.as_dict()

    def grid_batch_range_dev(self, dev_segments, t_lo, t_hi, out_ts_ptr, out_val_ptr, cap,
                             rows_ptr=None):
        n_out = C.c_uint64()
        metrics = _abi.GridMetricsC()
        self._check(self.lib.mdb_grid_batch_range_dev(
            self.handle, C.byref(dev_segments.seg), t_lo, t_hi, C.c_void_p(out_ts_ptr),
            C.c_void_p(out_val_ptr), C.c_void_p(rows_ptr), cap, C.byref(n_out), C.byref(metrics)))
        return n_out.value, metrics.as_dict()

    def grid_count_range_dev(self, dev_segments, t_lo, t_hi):
        n_out = C.c_uint64()
        self._check(self.lib.mdb_grid_count_range_dev(self.handle, C.byref(dev_segments.seg), t_lo,
                                                      t_hi, C.byref(n_out)))
        return n_out.value

    def grid_count_dev(self, dev_segments):
        n_out = C.c_uint64()
        self._check(self.lib.mdb_grid_count_dev(self.handle, C.byref(dev_segments.seg),
                                                C.byref(n_out)))
        return n_out.value

    def grid_batch_dev(self, dev_segments, out_ts_ptr, out_val_ptr, cap, rows_ptr=None):
        n_out = C.c_uint64()
        metrics = _abi.GridMetricsC()
        self._check(self.lib.mdb_grid_batch_dev(
            self.handle, C.byref(dev_segments.seg), C.c_void_p(out_ts_ptr), C.c_void_p(out_val_ptr),
            C.c_void_p(rows_ptr), cap, C.byref(n_out), C.byref(metrics)))
        return n_out.value, metrics.as_dict()

    def grid_resident(self, dev_segments, time_range=None):
        """grid() of a batch that is resident on the device into device columns, downloaded for the tests:
        (timestamps, values). The path a server with its segments in HBM takes (mdb_grid_batch[_range]_dev)."""
        if time_range is None:
            n = self.grid_count_dev(dev_segments)
        else:
            n = self.grid_count_range_dev(dev_segments, *time_range)
        out_ts, out_val = self.dev_alloc(8 * max(n, 1)), self.dev_alloc(4 * max(n, 1))
        try:
            if time_range is None:
                produced, _ = self.grid_batch_dev(dev_segments, out_ts, out_val, n)
            else:
                produced, _ = self.grid_batch_range_dev(dev_segments, time_range[0], time_range[1], out_ts, out_val, n)
            assert produced == n
            return self.download_array(out_ts, n, np.int64), self.download_array(out_val, n, np.float32)
        finally:
            self.dev_free(out_ts)
            self.dev_free(out_val)

    # ---- aggregates ------------------------------------------------------------------------------

    def agg_batch(self, batch, which_mask, state=None):
        seg = batch.as_c()
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch(self.handle, C.byref(seg), which_mask, C.byref(state)))
        return state

    def agg_batch_list(self, batches, which_mask, state=None):
        """Several host batches folded as one (mdb_agg_batch_list): what an accumulator that has gathered the batches
        of a run of update_batch calls passes."""
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * len(views))(*[C.pointer(view) for view in views])
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_list(self.handle, pointers, len(views), which_mask, C.byref(state)))
        return state

    def agg_batch_range(self, batch, t_lo, t_hi, which_mask, state=None):
        seg = batch.as_c()
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_range(self.handle, C.byref(seg), t_lo, t_hi, which_mask,
                                                 C.byref(state)))
        return state

    def agg_batch_range_list(self, batches, t_lo, t_hi, which_mask, state=None):
        """Several host batches folded as one under a time range (mdb_agg_batch_range_list): what the accumulators
        of a ranged query pass (rust/patches/0002)."""
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * len(views))(*[C.pointer(view) for view in views])
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_range_list(self.handle, pointers, len(views), t_lo, t_hi, which_mask,
                                                      C.byref(state)))
        return state

    def agg_batch_dev(self, dev_segments, which_mask, state=None):
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_dev(self.handle, C.byref(dev_segments.seg), which_mask,
                                               C.byref(state)))
        return state

    def agg_batch_range_dev(self, dev_segments, t_lo, t_hi, which_mask, state=None):
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_range_dev(self.handle, C.byref(dev_segments.seg), t_lo,
                                                     t_hi, which_mask, C.byref(state)))
        return state

    # ---- value filters (mdb_value_filter: see value_filter) ------------------------------------------

    def grid_filter(self, batch, flt, reserve_front=0):
        """grid() with a value predicate and a time range pushed down (mdb_grid_batch_filter_owned): only the passing
        rows cross PCIe. Returns copies (timestamps, values, rows_per_segment, metrics)."""
        seg = batch.as_c()
        out = C.POINTER(_abi.GridResultC)()
        self._check(self.lib.mdb_grid_batch_filter_owned(self.handle, C.byref(seg), C.byref(flt), int(reserve_front),
                                                         C.byref(out)))
        try:
            result = out.contents
            n, n_segments = int(result.n), int(result.n_segments)

            def copy_of(pointer, count, dtype):
                if count == 0:
                    return np.zeros(0, dtype=dtype)
                buffer = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(pointer)
                return np.frombuffer(buffer, dtype=dtype).copy()

            return (copy_of(result.timestamps, n, np.int64), copy_of(result.values, n, np.float32),
                    copy_of(result.rows_per_segment, n_segments, np.uint32), result.metrics.as_dict())
        finally:
            self.lib.mdb_grid_result_free(out)

    def grid_count_filter_dev(self, dev_segments, flt):
        n_out = C.c_uint64()
        self._check(self.lib.mdb_grid_count_filter_dev(self.handle, C.byref(dev_segments.seg), C.byref(flt),
                                                       C.byref(n_out)))
        return n_out.value

    def grid_filter_dev(self, dev_segments, flt, out_ts_ptr, out_val_ptr, cap, rows_ptr=None):
        """mdb_grid_batch_filter_dev into device columns; returns (rows produced, metrics)."""
        n_out = C.c_uint64()
        metrics = _abi.GridMetricsC()
        self._check(self.lib.mdb_grid_batch_filter_dev(
            self.handle, C.byref(dev_segments.seg), C.byref(flt), C.c_void_p(out_ts_ptr), C.c_void_p(out_val_ptr),
            C.c_void_p(rows_ptr), cap, C.byref(n_out), C.byref(metrics)))
        return n_out.value, metrics.as_dict()

    def grid_filter_resident(self, dev_segments, flt):
        """The dev form on a resident batch, downloaded: (timestamps, values, rows_per_segment, metrics)."""
        n = self.grid_count_filter_dev(dev_segments, flt)
        out_ts, out_val = self.dev_alloc(8 * max(n, 1)), self.dev_alloc(4 * max(n, 1))
        rows = self.dev_alloc(4 * max(len(dev_segments), 1))
        try:
            produced, metrics = self.grid_filter_dev(dev_segments, flt, out_ts, out_val, n, rows)
            assert produced == n
            return (self.download_array(out_ts, n, np.int64), self.download_array(out_val, n, np.float32),
                    self.download_array(rows, len(dev_segments), np.uint32), metrics)
        finally:
            for pointer in (out_ts, out_val, rows):
                self.dev_free(pointer)

    def agg_filter(self, batch, flt, which_mask, state=None):
        """COUNT / MIN / MAX / SUM of the points that pass `flt` (mdb_agg_batch_filter), folded into `state`."""
        seg = batch.as_c()
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_filter(self.handle, C.byref(seg), C.byref(flt), which_mask, C.byref(state)))
        return state

    def agg_filter_list(self, batches, flt, which_mask, state=None):
        """Several host batches folded as one (mdb_agg_batch_filter_list)."""
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_filter_list(self.handle, pointers, len(views), C.byref(flt), which_mask,
                                                       C.byref(state)))
        return state

    def agg_filter_dev(self, dev_segments, flt, which_mask, state=None):
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_filter_dev(self.handle, C.byref(dev_segments.seg), C.byref(flt), which_mask,
                                                      C.byref(state)))
        return state

    # ---- row masks: a predicate on one field selects the rows of another (mdb_mask_*, mdb_*_mask*, mdb_*_where*) ----

    def mask_filter_dev(self, dev_segments, flt, mask_ptr, cap_words, want_set=True):
        """mdb_mask_filter_dev: the mask of `flt` over the rows of the batch under the filter's time range, into
        `cap_words` device words at mask_ptr. Returns (n_rows, n_set) (n_set None unless want_set)."""
        n_rows, n_set = C.c_uint64(), C.c_uint64()
        self._check(self.lib.mdb_mask_filter_dev(self.handle, C.byref(dev_segments.seg), C.byref(flt), C.c_void_p(mask_ptr),
                                                 int(cap_words), C.byref(n_rows), C.byref(n_set) if want_set else None))
        return n_rows.value, (n_set.value if want_set else None)

    def mask_combine_dev(self, op, a_ptr, b_ptr, out_ptr, n_rows):
        """mdb_mask_combine_dev: out = a op b (MDB_MASK_*; b_ptr None for NOT); returns the set bits of out."""
        n_set = C.c_uint64()
        self._check(self.lib.mdb_mask_combine_dev(self.handle, int(op), C.c_void_p(a_ptr), C.c_void_p(b_ptr),
                                                  C.c_void_p(out_ptr), int(n_rows), C.byref(n_set)))
        return n_set.value

    def upload_mask(self, bits):
        """A bool array as a device mask (the padding bits zero); returns the pointer (dev_free it)."""
        bits = np.ascontiguousarray(bits, dtype=bool)
        packed = np.zeros(max(mask_words(len(bits)), 1) * 8, dtype=np.uint8)
        packed[: (len(bits) + 7) // 8] = np.packbits(bits, bitorder="little")
        return self.upload_array(packed)

    def download_mask(self, pointer, n_rows, with_padding=False):
        """A device mask as a bool array of n_rows entries (with_padding: of all 64 * words bits, padding included)."""
        words = mask_words(n_rows)
        if words == 0:
            return np.zeros(0, dtype=bool)
        raw = self.download_array(pointer, words * 8, np.uint8)
        return unpack_mask(raw, words * 64 if with_padding else n_rows)

    def grid_mask_dev(self, dev_segments, t_lo, t_hi, mask_ptr, n_rows, out_ts_ptr, out_val_ptr, cap, rows_ptr=None):
        """mdb_grid_batch_mask_dev into device columns (out_ts_ptr None: values only); returns (rows produced, metrics)."""
        n_out = C.c_uint64()
        metrics = _abi.GridMetricsC()
        self._check(self.lib.mdb_grid_batch_mask_dev(
            self.handle, C.byref(dev_segments.seg), int(t_lo), int(t_hi), C.c_void_p(mask_ptr), int(n_rows),
            C.c_void_p(out_ts_ptr), C.c_void_p(out_val_ptr), C.c_void_p(rows_ptr), int(cap), C.byref(n_out), C.byref(metrics)))
        return n_out.value, metrics.as_dict()

    def grid_mask_resident(self, dev_segments, t_lo, t_hi, mask_ptr, n_rows, n_set, values_only=False):
        """The dev form on a resident batch, downloaded: (timestamps or None, values, rows_per_segment, metrics).
        n_set: the set bits of the mask (the size of the output)."""
        out_ts = None if values_only else self.dev_alloc(8 * max(n_set, 1))
        out_val = self.dev_alloc(4 * max(n_set, 1))
        rows = self.dev_alloc(4 * max(len(dev_segments), 1))
        try:
            produced, metrics = self.grid_mask_dev(dev_segments, t_lo, t_hi, mask_ptr, n_rows, out_ts, out_val, n_set, rows)
            assert produced == n_set
            return (None if values_only else self.download_array(out_ts, n_set, np.int64),
                    self.download_array(out_val, n_set, np.float32),
                    self.download_array(rows, len(dev_segments), np.uint32), metrics)
        finally:
            for pointer in (out_ts, out_val, rows):
                if pointer is not None:
                    self.dev_free(pointer)

    def agg_mask_dev(self, dev_segments, t_lo, t_hi, mask_ptr, n_rows, which_mask, state=None):
        """mdb_agg_batch_mask_dev: the points the mask selects folded into `state`."""
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_mask_dev(self.handle, C.byref(dev_segments.seg), int(t_lo), int(t_hi),
                                                    C.c_void_p(mask_ptr), int(n_rows), which_mask, C.byref(state)))
        return state

    @staticmethod
    def _where_arguments(pred_batches, filters):
        if len(pred_batches) != len(filters):
            raise ValueError("one filter per predicate batch")
        views = {}
        for batch in pred_batches:  # (the same batch twice: the same mdb_segments pointer)
            if id(batch) not in views:
                views[id(batch)] = batch.as_c()
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(pred_batches), 1))(
            *[C.pointer(views[id(batch)]) for batch in pred_batches])
        array = (_abi.ValueFilterC * max(len(filters), 1))(*filters)
        return views, pointers, array

    def agg_where(self, pred_batches, filters, target, which_mask, state=None):
        """mdb_agg_batch_where: agg(target) WHERE filters[0](pred_batches[0]) AND ... over host batches."""
        views, pointers, array = self._where_arguments(pred_batches, filters)
        target_view = views.get(id(target)) or target.as_c()
        state = state or _abi.AggStateC.fresh()
        self._check(self.lib.mdb_agg_batch_where(self.handle, pointers, array, len(filters), C.byref(target_view),
                                                 which_mask, C.byref(state)))
        return state

    def grid_where(self, pred_batches, filters, target, values_only=False, reserve_front=0, flags=None):
        """mdb_grid_batch_where_owned: the rows of target WHERE ...; copies (timestamps or None, values,
        rows_per_segment, metrics)."""
        views, pointers, array = self._where_arguments(pred_batches, filters)
        target_view = views.get(id(target)) or target.as_c()
        if flags is None:
            flags = _abi.MDB_GRID_VALUES_ONLY if values_only else 0
        out = C.POINTER(_abi.GridResultC)()
        self._check(self.lib.mdb_grid_batch_where_owned(self.handle, pointers, array, len(filters), C.byref(target_view),
                                                        int(flags), int(reserve_front), C.byref(out)))
        try:
            result = out.contents
            n, n_segments = int(result.n), int(result.n_segments)

            def copy_of(pointer, count, dtype):
                if count == 0:
                    return np.zeros(0, dtype=dtype)
                buffer = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(pointer)
                return np.frombuffer(buffer, dtype=dtype).copy()

            return (copy_of(result.timestamps, n, np.int64) if result.timestamps else None,
                    copy_of(result.values, n, np.float32), copy_of(result.rows_per_segment, n_segments, np.uint32),
                    result.metrics.as_dict())
        finally:
            self.lib.mdb_grid_result_free(out)

    # ---- aggregates per time bucket ----------------------------------------------------------------

    @staticmethod
    def _bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, which_mask):
        return _abi.BucketRequestC(int(origin), int(width), int(n_buckets), INT64_MIN if t_lo is None else int(t_lo),
                                   INT64_MAX if t_hi is None else int(t_hi), int(n_groups), int(which_mask))

    @staticmethod
    def _bucket_states(states, n_groups, n_buckets):
        if states is None:
            return fresh_agg_states((n_groups, n_buckets))
        if states.dtype != AGG_STATE_DTYPE or states.shape != (n_groups, n_buckets) or not states.flags.c_contiguous:
            raise ValueError(f"states must be a contiguous ({n_groups}, {n_buckets}) array of AGG_STATE_DTYPE")
        return states

    @staticmethod
    def _groups_array(groups, n_rows):
        if groups is None:
            return None
        groups = np.ascontiguousarray(groups, dtype=np.uint32)
        if groups.shape != (n_rows,):
            raise ValueError(f"groups must hold one id per segment row ({n_rows})")
        return groups

    def agg_buckets(self, batch, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                    which_mask=_abi.MDB_AGG_COUNT | _abi.MDB_AGG_MIN | _abi.MDB_AGG_MAX | _abi.MDB_AGG_SUM,
                    states=None, n_groups=None):
        """COUNT / MIN / MAX / SUM per bucket of date_bin(width, ts, origin) and group (mdb_agg_buckets): returns
        `states` (or fresh ones), shape (n_groups, n_buckets), folded in place. `groups`: one id per segment row
        (None: all in group 0); n_groups defaults to states' rows, else to max(groups) + 1."""
        return self.agg_buckets_list([batch], origin, width, n_buckets, None if groups is None else [groups], t_lo,
                                     t_hi, which_mask, states, n_groups)

    def agg_buckets_list(self, batches, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                         which_mask=_abi.MDB_AGG_COUNT | _abi.MDB_AGG_MIN | _abi.MDB_AGG_MAX | _abi.MDB_AGG_SUM,
                         states=None, n_groups=None):
        """Several host batches folded as one (mdb_agg_buckets_list); `groups`: None or one array (or None) per batch."""
        return self._buckets_list(None, batches, origin, width, n_buckets, groups, t_lo, t_hi, which_mask, states,
                                  n_groups)

    def agg_buckets_dev(self, dev_segments, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                        which_mask=_abi.MDB_AGG_COUNT | _abi.MDB_AGG_MIN | _abi.MDB_AGG_MAX | _abi.MDB_AGG_SUM,
                        states=None, n_groups=None):
        """mdb_agg_buckets_dev on a resident batch: `groups` and `states` are uploaded, the states downloaded again."""
        return self._buckets_dev(None, dev_segments, origin, width, n_buckets, groups, t_lo, t_hi, which_mask, states,
                                 n_groups)

    def agg_buckets_filter(self, batch, flt, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                           which_mask=_abi.MDB_AGG_COUNT | _abi.MDB_AGG_MIN | _abi.MDB_AGG_MAX | _abi.MDB_AGG_SUM,
                           states=None, n_groups=None):
        """agg_buckets of the points that pass `flt`, an mdb_value_filter (value_filter), whose time range is ANDed
        with [t_lo, t_hi] (mdb_agg_buckets_filter)."""
        return self.agg_buckets_filter_list([batch], flt, origin, width, n_buckets,
                                            None if groups is None else [groups], t_lo, t_hi, which_mask, states,
                                            n_groups)

    def agg_buckets_filter_list(self, batches, flt, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                                which_mask=_abi.MDB_AGG_COUNT | _abi.MDB_AGG_MIN | _abi.MDB_AGG_MAX | _abi.MDB_AGG_SUM,
                                states=None, n_groups=None):
        """Several host batches folded as one (mdb_agg_buckets_filter_list)."""
        return self._buckets_list(flt, batches, origin, width, n_buckets, groups, t_lo, t_hi, which_mask, states,
                                  n_groups)

    def agg_buckets_filter_dev(self, dev_segments, flt, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                               which_mask=_abi.MDB_AGG_COUNT | _abi.MDB_AGG_MIN | _abi.MDB_AGG_MAX | _abi.MDB_AGG_SUM,
                               states=None, n_groups=None):
        """mdb_agg_buckets_filter_dev on a resident batch, as agg_buckets_dev."""
        return self._buckets_dev(flt, dev_segments, origin, width, n_buckets, groups, t_lo, t_hi, which_mask, states,
                                 n_groups)

    def _buckets_list(self, flt, batches, origin, width, n_buckets, groups, t_lo, t_hi, which_mask, states, n_groups):
        # (mdb_agg_buckets_list, or mdb_agg_buckets_filter_list when a filter is given)
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, states, batch_groups)
        states = self._bucket_states(states, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, which_mask)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        cells = states.ctypes.data_as(C.c_void_p)
        if flt is None:
            self._check(self.lib.mdb_agg_buckets_list(self.handle, pointers, group_pointers, len(views),
                                                      C.byref(request), cells))
        else:
            self._check(self.lib.mdb_agg_buckets_filter_list(self.handle, pointers, group_pointers, len(views),
                                                             C.byref(request), C.byref(flt), cells))
        return states

    def _buckets_dev(self, flt, dev_segments, origin, width, n_buckets, groups, t_lo, t_hi, which_mask, states,
                     n_groups):
        # (mdb_agg_buckets_dev, or mdb_agg_buckets_filter_dev when a filter is given)
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, states, [groups])
        states = self._bucket_states(states, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, which_mask)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_states = self.upload_array(states)
        try:
            group_pointer = None if dev_groups is None else C.c_void_p(dev_groups)
            if flt is None:
                self._check(self.lib.mdb_agg_buckets_dev(self.handle, C.byref(dev_segments.seg), group_pointer,
                                                         C.byref(request), C.c_void_p(dev_states)))
            else:
                self._check(self.lib.mdb_agg_buckets_filter_dev(self.handle, C.byref(dev_segments.seg), group_pointer,
                                                                C.byref(request), C.byref(flt), C.c_void_p(dev_states)))
            states[...] = self.download_array(dev_states, states.size, AGG_STATE_DTYPE).reshape(states.shape)
        finally:
            self.dev_free(dev_states)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return states

    # ---- M4 downsampling: first / last / min / max points per time bucket ----------------------------

    @staticmethod
    def _m4_cells(cells, n_groups, n_buckets):
        if cells is None:
            return fresh_m4_cells((n_groups, n_buckets))
        if cells.dtype != M4_CELL_DTYPE or cells.shape != (n_groups, n_buckets) or not cells.flags.c_contiguous:
            raise ValueError(f"cells must be a contiguous ({n_groups}, {n_buckets}) array of M4_CELL_DTYPE")
        return cells

    def m4_buckets(self, batch, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                   n_groups=None):
        """The first, last, lowest and highest point (with timestamps) and the count per bucket of
        date_bin(width, ts, origin) and group (mdb_m4_buckets): returns `cells` (or fresh ones), shape
        (n_groups, n_buckets), merged in place. `groups` and n_groups as for agg_buckets."""
        return self.m4_buckets_list([batch], origin, width, n_buckets, None if groups is None else [groups], t_lo,
                                    t_hi, cells, n_groups)

    def m4_buckets_list(self, batches, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                        n_groups=None):
        """Several host batches merged as one (mdb_m4_buckets_list); `groups`: None or one array (or None) per batch."""
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._m4_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_m4_buckets_list(self.handle, pointers, group_pointers, len(views), C.byref(request),
                                                 cells.ctypes.data_as(C.c_void_p)))
        return cells

    def m4_buckets_dev(self, dev_segments, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                       n_groups=None):
        """mdb_m4_buckets_dev on a resident batch: `groups` and `cells` are uploaded, the cells downloaded again."""
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._m4_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_m4_buckets_dev(self.handle, C.byref(dev_segments.seg),
                                                    None if dev_groups is None else C.c_void_p(dev_groups),
                                                    C.byref(request), C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, M4_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    # ---- variance and standard deviation: count, mean and m2 per time bucket --------------------------

    @staticmethod
    def _moments_cells(cells, n_groups, n_buckets):
        if cells is None:
            return fresh_moments_cells((n_groups, n_buckets))
        if cells.dtype != MOMENTS_CELL_DTYPE or cells.shape != (n_groups, n_buckets) or not cells.flags.c_contiguous:
            raise ValueError(f"cells must be a contiguous ({n_groups}, {n_buckets}) array of MOMENTS_CELL_DTYPE")
        return cells

    def moments_buckets(self, batch, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                        n_groups=None):
        """The count, the mean and m2 = sum((v - mean)^2) per bucket of date_bin(width, ts, origin) and group
        (mdb_moments_buckets): returns `cells` (or fresh ones), shape (n_groups, n_buckets), merged in place.
        `groups` and n_groups as for agg_buckets; moments_variance turns cells into variances."""
        return self.moments_buckets_list([batch], origin, width, n_buckets, None if groups is None else [groups],
                                         t_lo, t_hi, cells, n_groups)

    def moments_buckets_list(self, batches, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                             n_groups=None):
        """Several host batches merged as one (mdb_moments_buckets_list); `groups`: None or one array (or None) per
        batch."""
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._moments_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_moments_buckets_list(self.handle, pointers, group_pointers, len(views),
                                                      C.byref(request), cells.ctypes.data_as(C.c_void_p)))
        return cells

    def moments_buckets_dev(self, dev_segments, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                            cells=None, n_groups=None):
        """mdb_moments_buckets_dev on a resident batch: `groups` and `cells` are uploaded, the cells downloaded
        again."""
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._moments_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_moments_buckets_dev(self.handle, C.byref(dev_segments.seg),
                                                         None if dev_groups is None else C.c_void_p(dev_groups),
                                                         C.byref(request), C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, MOMENTS_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    def moments(self, batch, t_lo=None, t_hi=None, groups=None, n_groups=None):
        """The cells of the points of `batch` inside [t_lo, t_hi], one per group (shape (n_groups,)): one bucket over
        the data inside the range, what a whole-batch stddev / variance query needs."""
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(batch))])
        if len(batch) == 0:
            return fresh_moments_cells(n_groups)
        lo, hi = int(np.min(batch.start_time)), int(np.max(batch.end_time))
        lo = lo if t_lo is None else max(lo, int(t_lo))
        hi = hi if t_hi is None else min(hi, int(t_hi))
        if lo > hi:
            return fresh_moments_cells(n_groups)
        if hi - lo + 1 > INT64_MAX:
            raise ValueError("the data inside the range spans more than one bucket can hold: use moments_buckets")
        return self.moments_buckets(batch, lo, hi - lo + 1, 1, groups, lo, hi, None, n_groups).reshape(n_groups)

    # ---- covariance and correlation of two fields: count, means, m2 and c_xy per time bucket ----------

    @staticmethod
    def _comoments_cells(cells, n_groups, n_buckets):
        if cells is None:
            return fresh_comoments_cells((n_groups, n_buckets))
        if cells.dtype != COMOMENTS_CELL_DTYPE or cells.shape != (n_groups, n_buckets) or not cells.flags.c_contiguous:
            raise ValueError(f"cells must be a contiguous ({n_groups}, {n_buckets}) array of COMOMENTS_CELL_DTYPE")
        return cells

    def comoments_buckets(self, x, y, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                          n_groups=None):
        """The count, both means, both m2 and c_xy of the pairs (x, y) per bucket of date_bin(width, ts, origin) and
        group (mdb_comoments_buckets): x and y are two field batches of the same series that line up row for row.
        Returns `cells` (or fresh ones), shape (n_groups, n_buckets), merged in place. `groups` (per segment of x) and
        n_groups as for agg_buckets; comoments_finish turns cells into corr / covar_* / regr_*. `x is y` is uploaded
        once."""
        groups = self._groups_array(groups, len(x))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._comoments_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        x_view = x.as_c()
        y_view = x_view if y is x else y.as_c()
        self._check(self.lib.mdb_comoments_buckets(self.handle, C.byref(x_view), C.byref(y_view),
                                                   None if groups is None else groups.ctypes.data_as(C.c_void_p),
                                                   C.byref(request), cells.ctypes.data_as(C.c_void_p)))
        return cells

    def comoments_buckets_list(self, xs, ys, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                               n_groups=None):
        """Several host batches per field merged as one (mdb_comoments_buckets_list): the cuts of xs and ys need not
        coincide; `groups`: None or one array (or None) per batch of xs."""
        batch_groups = [None] * len(xs) if groups is None else [self._groups_array(g, len(b))
                                                                for g, b in zip(groups, xs)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._comoments_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        x_views = [batch.as_c() for batch in xs]
        y_views = [batch.as_c() for batch in ys]
        x_pointers = (C.POINTER(_abi.SegmentsC) * max(len(x_views), 1))(*[C.pointer(view) for view in x_views])
        y_pointers = (C.POINTER(_abi.SegmentsC) * max(len(y_views), 1))(*[C.pointer(view) for view in y_views])
        group_pointers = (C.c_void_p * max(len(x_views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_comoments_buckets_list(self.handle, x_pointers, len(x_views), y_pointers, len(y_views),
                                                        group_pointers, C.byref(request),
                                                        cells.ctypes.data_as(C.c_void_p)))
        return cells

    def comoments_buckets_dev(self, dev_x, dev_y, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                              cells=None, n_groups=None):
        """mdb_comoments_buckets_dev on two resident batches: `groups` and `cells` are uploaded, the cells downloaded
        again."""
        groups = self._groups_array(groups, len(dev_x))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._comoments_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_comoments_buckets_dev(self.handle, C.byref(dev_x.seg), C.byref(dev_y.seg),
                                                           None if dev_groups is None else C.c_void_p(dev_groups),
                                                           C.byref(request), C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, COMOMENTS_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    def comoments(self, x, y, t_lo=None, t_hi=None, groups=None, n_groups=None):
        """The cells of the pairs of `x` and `y` inside [t_lo, t_hi], one per group (shape (n_groups,)): one bucket
        over the data inside the range, what a whole-batch corr / covar / regr query needs."""
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(x))])
        if len(x) == 0:
            return fresh_comoments_cells(n_groups)
        lo, hi = int(np.min(x.start_time)), int(np.max(x.end_time))
        lo = lo if t_lo is None else max(lo, int(t_lo))
        hi = hi if t_hi is None else min(hi, int(t_hi))
        if lo > hi:
            return fresh_comoments_cells(n_groups)
        if hi - lo + 1 > INT64_MAX:
            raise ValueError("the data inside the range spans more than one bucket can hold: use comoments_buckets")
        return self.comoments_buckets(x, y, lo, hi - lo + 1, 1, groups, lo, hi, None, n_groups).reshape(n_groups)

    # ---- derived fields of two fields: z = f(x, y) as a column and count, mean, m2, min, max per time bucket ----------

    @staticmethod
    def _derived_cells(cells, n_groups, n_buckets):
        if cells is None:
            return fresh_derived_cells((n_groups, n_buckets))
        if cells.dtype != DERIVED_CELL_DTYPE or cells.shape != (n_groups, n_buckets) or not cells.flags.c_contiguous:
            raise ValueError(f"cells must be a contiguous ({n_groups}, {n_buckets}) array of DERIVED_CELL_DTYPE")
        return cells

    def derived_values(self, x, y, expr, t_lo=None, t_hi=None, timestamps=True):
        """The generated column z = f(x, y) of two host batches that line up row for row (mdb_derived_values): the rows
        of grid_batch_range(x, t_lo, t_hi) paired with those of y. Returns (timestamps of x or None, z as float32)."""
        t_lo = INT64_MIN if t_lo is None else int(t_lo)
        t_hi = INT64_MAX if t_hi is None else int(t_hi)
        expr = derived_expr(expr)
        x_view = x.as_c()
        y_view = x_view if y is x else y.as_c()
        n_out = C.c_uint64()
        self._check(self.lib.mdb_grid_count_range(self.handle, C.byref(x_view), t_lo, t_hi, C.byref(n_out)))
        capacity = n_out.value
        out_ts = np.empty(capacity, dtype=np.int64) if timestamps else None
        out_val = np.empty(capacity, dtype=np.float32)
        self._check(self.lib.mdb_derived_values(self.handle, C.byref(x_view), C.byref(y_view), C.byref(expr), t_lo, t_hi,
                                                None if out_ts is None else out_ts.ctypes.data_as(C.c_void_p),
                                                out_val.ctypes.data_as(C.c_void_p), capacity, C.byref(n_out)))
        return (None if out_ts is None else out_ts[:n_out.value]), out_val[:n_out.value]

    def derived_values_dev(self, dev_x, dev_y, expr, t_lo, t_hi, out_ts_ptr, out_val_ptr, capacity):
        """mdb_derived_values_dev on two resident batches into device arrays (out_ts_ptr may be None; out_val_ptr needs
        4-byte alignment only). Returns the row count."""
        expr = derived_expr(expr)
        n_out = C.c_uint64()
        self._check(self.lib.mdb_derived_values_dev(self.handle, C.byref(dev_x.seg), C.byref(dev_y.seg), C.byref(expr),
                                                    int(t_lo), int(t_hi), C.c_void_p(out_ts_ptr), C.c_void_p(out_val_ptr),
                                                    capacity, C.byref(n_out)))
        return n_out.value

    def derived_buckets(self, x, y, expr, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                        n_groups=None):
        """The count, mean, m2, min and max of z = f(x, y) per bucket of date_bin(width, ts, origin) and group
        (mdb_derived_buckets): x and y are two field batches of the same series that line up row for row. Returns
        `cells` (or fresh ones), shape (n_groups, n_buckets), merged in place. `groups` (per segment of x) and n_groups
        as for agg_buckets; derived_stats gives what moments_variance takes. `x is y` is uploaded once."""
        groups = self._groups_array(groups, len(x))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._derived_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        expr = derived_expr(expr)
        x_view = x.as_c()
        y_view = x_view if y is x else y.as_c()
        self._check(self.lib.mdb_derived_buckets(self.handle, C.byref(x_view), C.byref(y_view),
                                                 None if groups is None else groups.ctypes.data_as(C.c_void_p),
                                                 C.byref(request), C.byref(expr), cells.ctypes.data_as(C.c_void_p)))
        return cells

    def derived_buckets_list(self, xs, ys, expr, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                             n_groups=None):
        """Several host batches per field merged as one (mdb_derived_buckets_list): the cuts of xs and ys need not
        coincide; `groups`: None or one array (or None) per batch of xs."""
        batch_groups = [None] * len(xs) if groups is None else [self._groups_array(g, len(b))
                                                                for g, b in zip(groups, xs)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._derived_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        expr = derived_expr(expr)
        x_views = [batch.as_c() for batch in xs]
        y_views = x_views if all(a is b for a, b in zip(xs, ys)) and len(xs) == len(ys) else [batch.as_c() for batch in ys]
        x_pointers = (C.POINTER(_abi.SegmentsC) * max(len(x_views), 1))(*[C.pointer(view) for view in x_views])
        y_pointers = (C.POINTER(_abi.SegmentsC) * max(len(y_views), 1))(*[C.pointer(view) for view in y_views])
        group_pointers = (C.c_void_p * max(len(x_views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_derived_buckets_list(self.handle, x_pointers, len(x_views), y_pointers, len(y_views),
                                                      group_pointers, C.byref(request), C.byref(expr),
                                                      cells.ctypes.data_as(C.c_void_p)))
        return cells

    def derived_buckets_dev(self, dev_x, dev_y, expr, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                            cells=None, n_groups=None):
        """mdb_derived_buckets_dev on two resident batches: `groups` and `cells` are uploaded, the cells downloaded
        again."""
        groups = self._groups_array(groups, len(dev_x))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._derived_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        expr = derived_expr(expr)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_derived_buckets_dev(self.handle, C.byref(dev_x.seg), C.byref(dev_y.seg),
                                                         None if dev_groups is None else C.c_void_p(dev_groups),
                                                         C.byref(request), C.byref(expr), C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, DERIVED_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    def derived(self, x, y, expr, t_lo=None, t_hi=None, groups=None, n_groups=None):
        """The cells of z = f(x, y) inside [t_lo, t_hi], one per group (shape (n_groups,)): one bucket over the data
        inside the range, what a whole-batch MIN / MAX / AVG / variance of a generated field needs."""
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(x))])
        if len(x) == 0:
            return fresh_derived_cells(n_groups)
        lo, hi = int(np.min(x.start_time)), int(np.max(x.end_time))
        lo = lo if t_lo is None else max(lo, int(t_lo))
        hi = hi if t_hi is None else min(hi, int(t_hi))
        if lo > hi:
            return fresh_derived_cells(n_groups)
        if hi - lo + 1 > INT64_MAX:
            raise ValueError("the data inside the range spans more than one bucket can hold: use derived_buckets")
        return self.derived_buckets(x, y, expr, lo, hi - lo + 1, 1, groups, lo, hi, None, n_groups).reshape(n_groups)

    # ---- rolling windows over per-bucket cells: moving aggregates -------------------------------------------------

    def roll_cells_dev(self, kind, cells_ptr, n_outer, n_buckets, n_inner, window, stride, out_ptr, capacity):
        """mdb_roll_cells_dev: the cells [n_outer][n_buckets][n_inner] at `cells_ptr` (HBM, 8-byte aligned) rolled into
        [n_outer][n_windows][n_inner] cells at `out_ptr` (HBM, room for `capacity` cells), enqueued on the context's
        stream: the bytes roll_cells gives. Returns the number of windows per column."""
        request = _abi.RollRequestC(int(kind), 0, int(n_outer), int(n_buckets), int(n_inner), int(window), int(stride))
        self._check(self.lib.mdb_roll_cells_dev(self.handle, C.byref(request), C.c_void_p(cells_ptr), C.c_void_p(out_ptr),
                                                int(capacity)))
        n_windows = C.c_uint64()
        self._check(self.lib.mdb_roll_windows(C.byref(request), C.byref(n_windows)))
        return n_windows.value

    # ---- linear trend of a field over time: comoments cells with x = the time offset inside the bucket ----------

    def trend_buckets(self, batch, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                      n_groups=None):
        """The trend of one field over time per bucket of date_bin(width, ts, origin) and group (mdb_trend_buckets):
        cells of COMOMENTS_CELL_DTYPE with x = the time offset of a point inside its bucket (microseconds, in
        [0, width)) and y = its value. Returns `cells` (or fresh ones), shape (n_groups, n_buckets), merged in place.
        `groups` and n_groups as for agg_buckets; comoments_finish gives regr_slope (per microsecond), regr_r2, corr
        and covar_*, and "regr_intercept" the fitted value at the bucket's first instant."""
        return self.trend_buckets_list([batch], origin, width, n_buckets, None if groups is None else [groups],
                                       t_lo, t_hi, cells, n_groups)

    def trend_buckets_list(self, batches, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                           n_groups=None):
        """Several host batches merged as one (mdb_trend_buckets_list); `groups`: None or one array (or None) per
        batch."""
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._comoments_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_trend_buckets_list(self.handle, pointers, group_pointers, len(views),
                                                    C.byref(request), cells.ctypes.data_as(C.c_void_p)))
        return cells

    def trend_buckets_dev(self, dev_segments, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                          cells=None, n_groups=None):
        """mdb_trend_buckets_dev on a resident batch: `groups` and `cells` are uploaded, the cells downloaded again."""
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._comoments_cells(cells, n_groups, n_buckets)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_trend_buckets_dev(self.handle, C.byref(dev_segments.seg),
                                                       None if dev_groups is None else C.c_void_p(dev_groups),
                                                       C.byref(request), C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, COMOMENTS_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    def trend(self, batch, t_lo=None, t_hi=None, groups=None, n_groups=None, origin=None):
        """(cells, origin): the trend cells of the points of `batch` inside [t_lo, t_hi], one per group (shape
        (n_groups,)) - one bucket over the data inside the range - and the instant x is counted from. By default that
        is the first instant of the bucket (the first timestamp the range can hold); it is returned so the caller can
        place the line: value(t) = regr_intercept + regr_slope * (t - origin). A given `origin` must not lie behind
        that instant."""
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(batch))])
        if len(batch) == 0:
            return fresh_comoments_cells(n_groups), 0 if origin is None else int(origin)
        lo, hi = int(np.min(batch.start_time)), int(np.max(batch.end_time))
        lo = lo if t_lo is None else max(lo, int(t_lo))
        hi = hi if t_hi is None else min(hi, int(t_hi))
        origin = lo if origin is None else int(origin)
        if lo > hi:
            return fresh_comoments_cells(n_groups), origin
        if origin > lo:
            raise ValueError("origin must not lie behind the first instant of the data inside the range")
        if hi - origin + 1 > INT64_MAX:
            raise ValueError("the data inside the range spans more than one bucket can hold: use trend_buckets")
        cells = self.trend_buckets(batch, origin, hi - origin + 1, 1, groups, lo, hi, None, n_groups)
        return cells.reshape(n_groups), origin

    # ---- time-weighted averages and integrals: the series as a function of time per bucket --------------------------

    @staticmethod
    def _integral_cells(cells, n_groups, n_buckets):
        if cells is None:
            return fresh_integral_cells((n_groups, n_buckets))
        if cells.dtype != INTEGRAL_CELL_DTYPE or cells.shape != (n_groups, n_buckets) or not cells.flags.c_contiguous:
            raise ValueError(f"cells must be a contiguous ({n_groups}, {n_buckets}) array of INTEGRAL_CELL_DTYPE")
        return cells

    @classmethod
    def _integral_request(cls, origin, width, n_buckets, n_groups, method, max_gap):
        request = _abi.IntegralRequestC()
        request.buckets = cls._bucket_request(origin, width, n_buckets, n_groups, None, None, 0)
        request.max_gap = INT64_MAX if max_gap is None else int(max_gap)
        request.method = int(method)
        request.flags = 0
        return request

    def integral_buckets(self, batch, origin, width, n_buckets, groups=None, method=MDB_INTEGRAL_LINEAR, max_gap=None,
                         cells=None, n_groups=None):
        """The defined time and the integral of one field per bucket [origin + b * width, origin + (b + 1) * width)
        and group (mdb_integral_buckets): cells of INTEGRAL_CELL_DTYPE, duration in microseconds, integral in
        value x microseconds; integral_average gives the time-weighted average. Between two linked rows - same group,
        time moving forward, at most max_gap apart (None: no gap rule) - the value is interpolated
        (MDB_INTEGRAL_LINEAR) or the earlier one carried forward (MDB_INTEGRAL_STEP). Returns `cells` (or fresh ones),
        shape (n_groups, n_buckets), merged in place. `groups` and n_groups as for agg_buckets. Links do not cross
        calls: cut batches at series boundaries."""
        return self.integral_buckets_list([batch], origin, width, n_buckets, None if groups is None else [groups],
                                          method, max_gap, cells, n_groups)

    def integral_buckets_list(self, batches, origin, width, n_buckets, groups=None, method=MDB_INTEGRAL_LINEAR,
                              max_gap=None, cells=None, n_groups=None):
        """Several host batches merged as one (mdb_integral_buckets_list): a link may cross from one batch to the next;
        `groups`: None or one array (or None) per batch."""
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._integral_cells(cells, n_groups, n_buckets)
        request = self._integral_request(origin, width, n_buckets, n_groups, method, max_gap)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_integral_buckets_list(self.handle, pointers, group_pointers, len(views),
                                                       C.byref(request), cells.ctypes.data_as(C.c_void_p)))
        return cells

    def integral_buckets_dev(self, dev_segments, origin, width, n_buckets, groups=None, method=MDB_INTEGRAL_LINEAR,
                             max_gap=None, cells=None, n_groups=None):
        """mdb_integral_buckets_dev on a resident batch: `groups` and `cells` are uploaded, the cells downloaded
        again."""
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._integral_cells(cells, n_groups, n_buckets)
        request = self._integral_request(origin, width, n_buckets, n_groups, method, max_gap)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_integral_buckets_dev(self.handle, C.byref(dev_segments.seg),
                                                          None if dev_groups is None else C.c_void_p(dev_groups),
                                                          C.byref(request), C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, INTEGRAL_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    def integral(self, batch, groups=None, n_groups=None, method=MDB_INTEGRAL_LINEAR, max_gap=None):
        """The cells of `batch` as one bucket over its span, one per group (shape (n_groups,)): what a whole-batch
        time-weighted average or integral needs."""
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(batch))])
        if len(batch) == 0:
            return fresh_integral_cells(n_groups)
        lo = int(min(np.min(batch.start_time), np.min(batch.end_time)))
        hi = int(max(np.max(batch.start_time), np.max(batch.end_time)))
        if hi - lo + 1 > INT64_MAX:
            raise ValueError("the batch spans more than one bucket can hold: use integral_buckets")
        return self.integral_buckets(batch, lo, hi - lo + 1, 1, groups, method, max_gap, None, n_groups).reshape(n_groups)

    # ---- changes between consecutive points per bucket: increase, restarts, ramps, total variation ---------------

    @staticmethod
    def _change_cells(cells, n_groups, n_buckets):
        if cells is None:
            return fresh_change_cells((n_groups, n_buckets))
        if cells.dtype != CHANGE_CELL_DTYPE or cells.shape != (n_groups, n_buckets) or not cells.flags.c_contiguous:
            raise ValueError(f"cells must be a contiguous ({n_groups}, {n_buckets}) array of CHANGE_CELL_DTYPE")
        return cells

    @classmethod
    def _change_request(cls, origin, width, n_buckets, n_groups, max_gap, reserved=0, flags=0):
        request = _abi.ChangeRequestC()
        request.buckets = cls._bucket_request(origin, width, n_buckets, n_groups, None, None, 0)
        request.max_gap = INT64_MAX if max_gap is None else int(max_gap)
        request.reserved = int(reserved)
        request.flags = int(flags)
        return request

    def change_buckets(self, batch, origin, width, n_buckets, groups=None, max_gap=None, cells=None, n_groups=None):
        """The changes between consecutive rows of one field per bucket [origin + b * width, origin + (b + 1) * width)
        and group (mdb_change_buckets): cells of CHANGE_CELL_DTYPE. Two consecutive rows are linked when they share a
        group, time moves forward and they are at most max_gap apart (None: no gap rule); a linked pair belongs to the
        bucket of its later row. change_finish gives the net change, the total variation, the increase of a counter
        and its rate. Returns `cells` (or fresh ones), shape (n_groups, n_buckets), merged in place. `groups` and
        n_groups as for agg_buckets. Links do not cross calls: cut batches at series boundaries."""
        return self.change_buckets_list([batch], origin, width, n_buckets, None if groups is None else [groups],
                                        max_gap, cells, n_groups)

    def change_buckets_list(self, batches, origin, width, n_buckets, groups=None, max_gap=None, cells=None,
                            n_groups=None):
        """Several host batches merged as one (mdb_change_buckets_list): a link may cross from one batch to the next;
        `groups`: None or one array (or None) per batch."""
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._change_cells(cells, n_groups, n_buckets)
        request = self._change_request(origin, width, n_buckets, n_groups, max_gap)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_change_buckets_list(self.handle, pointers, group_pointers, len(views),
                                                     C.byref(request), cells.ctypes.data_as(C.c_void_p)))
        return cells

    def change_buckets_dev(self, dev_segments, origin, width, n_buckets, groups=None, max_gap=None, cells=None,
                           n_groups=None):
        """mdb_change_buckets_dev on a resident batch: `groups` and `cells` are uploaded, the cells downloaded again."""
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._change_cells(cells, n_groups, n_buckets)
        request = self._change_request(origin, width, n_buckets, n_groups, max_gap)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_change_buckets_dev(self.handle, C.byref(dev_segments.seg),
                                                        None if dev_groups is None else C.c_void_p(dev_groups),
                                                        C.byref(request), C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, CHANGE_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    def change(self, batch, groups=None, n_groups=None, max_gap=None):
        """The cells of `batch` as one bucket over its span, one per group (shape (n_groups,)): what a whole-batch
        increase, restart count or total variation needs."""
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(batch))])
        if len(batch) == 0:
            return fresh_change_cells(n_groups)
        lo = int(min(np.min(batch.start_time), np.min(batch.end_time)))
        hi = int(max(np.max(batch.start_time), np.max(batch.end_time)))
        if hi - lo + 1 > INT64_MAX:
            raise ValueError("the batch spans more than one bucket can hold: use change_buckets")
        return self.change_buckets(batch, lo, hi - lo + 1, 1, groups, max_gap, None, n_groups).reshape(n_groups)

    # ---- dwell: the time spent per value cell, per bucket ---------------------------------------------------------

    @classmethod
    def _dwell_request(cls, origin, width, n_buckets, n_groups, max_gap, method=MDB_DWELL_STEP, flags=0):
        request = _abi.DwellRequestC()
        request.buckets = cls._bucket_request(origin, width, n_buckets, n_groups, None, None, 0)
        request.max_gap = INT64_MAX if max_gap is None else int(max_gap)
        request.method = int(method)
        request.flags = int(flags)
        return request

    def dwell_buckets(self, batch, edges, origin, width, n_buckets, groups=None, max_gap=None, dwell=None, n_groups=None):
        """The microseconds one field spent in each value cell, ADDED to `dwell` (or to fresh zeros), shape (n_groups,
        n_buckets, len(edges) + 1), per bucket [origin + b * width, origin + (b + 1) * width) and group
        (mdb_dwell_buckets). Between two linked rows - same group, time moving forward, at most max_gap apart (None: no
        gap rule) - the earlier value is held up to the later row; the cells are those of hist_buckets. dwell_share
        gives the share of each row's linked time. `groups` and n_groups as for agg_buckets. Links do not cross calls:
        cut batches at series boundaries."""
        return self.dwell_buckets_list([batch], edges, origin, width, n_buckets, None if groups is None else [groups],
                                       max_gap, dwell, n_groups)

    def dwell_buckets_list(self, batches, edges, origin, width, n_buckets, groups=None, max_gap=None, dwell=None,
                           n_groups=None):
        """Several host batches as one (mdb_dwell_buckets_list): a link may cross from one batch to the next; `groups`:
        None or one array (or None) per batch."""
        edges = _edges_array(edges)
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, dwell, batch_groups)
        dwell = self._hist_bucket_counts(dwell, n_groups, n_buckets, len(edges) + 1)
        request = self._dwell_request(origin, width, n_buckets, n_groups, max_gap)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_dwell_buckets_list(self.handle, pointers, group_pointers, len(views), C.byref(request),
                                                    edges.ctypes.data_as(C.c_void_p), len(edges),
                                                    dwell.ctypes.data_as(C.c_void_p)))
        return dwell

    def dwell_buckets_dev(self, dev_segments, edges, origin, width, n_buckets, groups=None, max_gap=None, dwell=None,
                          n_groups=None):
        """mdb_dwell_buckets_dev on a resident batch: `groups` and `dwell` are uploaded, the counters downloaded again."""
        edges = _edges_array(edges)
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, dwell, [groups])
        dwell = self._hist_bucket_counts(dwell, n_groups, n_buckets, len(edges) + 1)
        request = self._dwell_request(origin, width, n_buckets, n_groups, max_gap)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_dwell = self.upload_array(dwell)
        try:
            self._check(self.lib.mdb_dwell_buckets_dev(self.handle, C.byref(dev_segments.seg),
                                                       None if dev_groups is None else C.c_void_p(dev_groups),
                                                       C.byref(request), edges.ctypes.data_as(C.c_void_p), len(edges),
                                                       C.c_void_p(dev_dwell)))
            dwell[...] = self.download_array(dev_dwell, dwell.size, np.uint64).reshape(dwell.shape)
        finally:
            self.dev_free(dev_dwell)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return dwell

    def dwell(self, batch, edges, groups=None, n_groups=None, max_gap=None):
        """The microseconds per value cell of `batch` as one bucket over its span, per group (shape (n_groups,
        len(edges) + 1)): time in state of a whole batch."""
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(batch))])
        if len(batch) == 0:
            return np.zeros((n_groups, len(_edges_array(edges)) + 1), dtype=np.uint64)
        lo = int(min(np.min(batch.start_time), np.min(batch.end_time)))
        hi = int(max(np.max(batch.start_time), np.max(batch.end_time)))
        if hi - lo + 1 > INT64_MAX:
            raise ValueError("the batch spans more than one bucket can hold: use dwell_buckets")
        return self.dwell_buckets(batch, edges, lo, hi - lo + 1, 1, groups, max_gap, None, n_groups).reshape(n_groups, -1)

    # ---- transit: transitions between value cells, per bucket ------------------------------------------------------

    @classmethod
    def _transit_request(cls, origin, width, n_buckets, n_groups, max_gap, reserved=0, flags=0):
        request = _abi.TransitRequestC()
        request.buckets = cls._bucket_request(origin, width, n_buckets, n_groups, None, None, 0)
        request.max_gap = INT64_MAX if max_gap is None else int(max_gap)
        request.reserved = int(reserved)
        request.flags = int(flags)
        return request

    @staticmethod
    def _transit_counts(counts, n_groups, n_buckets, n_cells):
        if counts is None:
            return np.zeros((n_groups, n_buckets, n_cells, n_cells), dtype=np.uint64)
        shape = (n_groups, n_buckets, n_cells, n_cells)
        if counts.dtype != np.uint64 or counts.shape != shape or not counts.flags.c_contiguous:
            raise ValueError(f"counts must be a contiguous {shape} array of uint64")
        return counts

    def transit_buckets(self, batch, edges, origin, width, n_buckets, groups=None, max_gap=None, counts=None,
                        n_groups=None):
        """The linked pairs of rows of one field by the value cells they go from and to, ADDED to `counts` (or to fresh
        zeros), shape (n_groups, n_buckets, len(edges) + 1, len(edges) + 1) indexed [from][to], per bucket [origin + b *
        width, origin + (b + 1) * width) and group (mdb_transit_buckets). Two rows are linked when they share a group,
        time moves forward and they are at most max_gap apart (None: no gap rule); a pair belongs to the bucket of its
        later row; the cells are those of hist_buckets. transit_crossings gives the crossings of each edge. `groups`
        and n_groups as for agg_buckets. Links do not cross calls: cut batches at series boundaries."""
        return self.transit_buckets_list([batch], edges, origin, width, n_buckets, None if groups is None else [groups],
                                         max_gap, counts, n_groups)

    def transit_buckets_list(self, batches, edges, origin, width, n_buckets, groups=None, max_gap=None, counts=None,
                             n_groups=None):
        """Several host batches as one (mdb_transit_buckets_list): a pair may cross from one batch to the next;
        `groups`: None or one array (or None) per batch."""
        edges = _edges_array(edges)
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, counts, batch_groups)
        counts = self._transit_counts(counts, n_groups, n_buckets, len(edges) + 1)
        request = self._transit_request(origin, width, n_buckets, n_groups, max_gap)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_transit_buckets_list(self.handle, pointers, group_pointers, len(views),
                                                      C.byref(request), edges.ctypes.data_as(C.c_void_p), len(edges),
                                                      counts.ctypes.data_as(C.c_void_p)))
        return counts

    def transit_buckets_dev(self, dev_segments, edges, origin, width, n_buckets, groups=None, max_gap=None, counts=None,
                            n_groups=None):
        """mdb_transit_buckets_dev on a resident batch: `groups` and `counts` are uploaded, the counters downloaded
        again."""
        edges = _edges_array(edges)
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, counts, [groups])
        counts = self._transit_counts(counts, n_groups, n_buckets, len(edges) + 1)
        request = self._transit_request(origin, width, n_buckets, n_groups, max_gap)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_counts = self.upload_array(counts)
        try:
            self._check(self.lib.mdb_transit_buckets_dev(self.handle, C.byref(dev_segments.seg),
                                                         None if dev_groups is None else C.c_void_p(dev_groups),
                                                         C.byref(request), edges.ctypes.data_as(C.c_void_p), len(edges),
                                                         C.c_void_p(dev_counts)))
            counts[...] = self.download_array(dev_counts, counts.size, np.uint64).reshape(counts.shape)
        finally:
            self.dev_free(dev_counts)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return counts

    def transit(self, batch, edges, groups=None, n_groups=None, max_gap=None):
        """The transitions of `batch` as one bucket over its span, per group (shape (n_groups, len(edges) + 1,
        len(edges) + 1), indexed [from][to]): the state-transition matrix of a whole batch."""
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(batch))])
        n_cells = len(_edges_array(edges)) + 1
        if len(batch) == 0:
            return np.zeros((n_groups, n_cells, n_cells), dtype=np.uint64)
        lo = int(min(np.min(batch.start_time), np.min(batch.end_time)))
        hi = int(max(np.max(batch.start_time), np.max(batch.end_time)))
        if hi - lo + 1 > INT64_MAX:
            raise ValueError("the batch spans more than one bucket can hold: use transit_buckets")
        return self.transit_buckets(batch, edges, lo, hi - lo + 1, 1, groups, max_gap, None, n_groups).reshape(
            n_groups, n_cells, n_cells)

    # ---- sampling: the value of a series at regular instants (gap-fill, LOCF, interpolation) --------------------

    @staticmethod
    def _sample_cells(cells, n_groups, n_instants):
        if cells is None:
            return fresh_sample_cells((n_groups, n_instants))
        if cells.dtype != SAMPLE_CELL_DTYPE or cells.shape != (n_groups, n_instants) or not cells.flags.c_contiguous:
            raise ValueError(f"cells must be a contiguous ({n_groups}, {n_instants}) array of SAMPLE_CELL_DTYPE")
        return cells

    @classmethod
    def _sample_request(cls, origin, width, n_instants, n_groups, method, max_gap):
        request = _abi.SampleRequestC()
        request.instants = cls._bucket_request(origin, width, n_instants, n_groups, None, None, 0)
        request.max_gap = INT64_MAX if max_gap is None else int(max_gap)
        request.method = int(method)
        request.flags = 0
        return request

    def sample_at(self, batch, origin, width, n_instants, groups=None, method=MDB_SAMPLE_LINEAR, max_gap=None,
                  cells=None, n_groups=None):
        """The value of one field at the instants origin + k * width, k < n_instants, per group (mdb_sample_at): cells
        of SAMPLE_CELL_DTYPE; sample_values gives sum / count, NaN where nothing reaches an instant. A row on an
        instant contributes its value; between two linked rows - same group, time moving forward, at most max_gap
        apart (None: no gap rule) - the value is interpolated (MDB_SAMPLE_LINEAR) or the earlier one carried forward
        (MDB_SAMPLE_STEP); MDB_SAMPLE_EXACT takes rows only. Returns `cells` (or fresh ones), shape (n_groups,
        n_instants), merged in place. `groups` and n_groups as for agg_buckets. Links do not cross calls: cut batches
        at series boundaries."""
        return self.sample_at_list([batch], origin, width, n_instants, None if groups is None else [groups], method,
                                   max_gap, cells, n_groups)

    def sample_at_list(self, batches, origin, width, n_instants, groups=None, method=MDB_SAMPLE_LINEAR, max_gap=None,
                       cells=None, n_groups=None):
        """Several host batches sampled as one (mdb_sample_at_list): a link may cross from one batch to the next;
        `groups`: None or one array (or None) per batch."""
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._sample_cells(cells, n_groups, n_instants)
        request = self._sample_request(origin, width, n_instants, n_groups, method, max_gap)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_sample_at_list(self.handle, pointers, group_pointers, len(views), C.byref(request),
                                                cells.ctypes.data_as(C.c_void_p)))
        return cells

    def sample_at_dev(self, dev_segments, origin, width, n_instants, groups=None, method=MDB_SAMPLE_LINEAR,
                      max_gap=None, cells=None, n_groups=None):
        """mdb_sample_at_dev on a resident batch: `groups` and `cells` are uploaded, the cells downloaded again."""
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._sample_cells(cells, n_groups, n_instants)
        request = self._sample_request(origin, width, n_instants, n_groups, method, max_gap)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_sample_at_dev(self.handle, C.byref(dev_segments.seg),
                                                   None if dev_groups is None else C.c_void_p(dev_groups),
                                                   C.byref(request), C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, SAMPLE_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    # ---- episodes: the maximal runs of points that pass a value predicate ----------------------------------------

    @staticmethod
    def _episodes_request(flt, n_groups, max_gap, min_duration, min_count):
        request = _abi.EpisodesRequestC()
        C.memmove(C.addressof(request), C.addressof(flt), C.sizeof(_abi.ValueFilterC))
        request.max_gap = INT64_MAX if max_gap is None else int(max_gap)
        request.min_duration = int(min_duration)
        request.min_count = int(min_count)
        request.n_groups = int(n_groups)
        request.flags = 0
        return request

    def episodes(self, batch, flt, groups=None, n_groups=None, max_gap=None, min_duration=0, min_count=0):
        """(episodes, n_rows, n_passing): the maximal runs of rows of `batch` that pass `flt` (value_filter(...): value
        bounds and time range), each row continuing its predecessor - same group, time not stepping back, at most
        max_gap later (None: no gap rule) - as a structured array of EPISODE_DTYPE ordered by first_row
        (mdb_episodes). Rows are numbered as the masks number them. Only episodes of at least min_count rows and
        min_duration microseconds are reported; n_passing counts every passing row. `groups`: one id per segment row
        (None: all in group 0)."""
        return self.episodes_list([batch], flt, None if groups is None else [groups], n_groups, max_gap, min_duration,
                                  min_count)

    def episodes_list(self, batches, flt, groups=None, n_groups=None, max_gap=None, min_duration=0, min_count=0):
        """Several host batches folded as one (mdb_episodes_list): an episode may cross from one batch to the next,
        first_segment counts through the list. `groups`: None or one array (or None) per batch."""
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        request = self._episodes_request(flt, self._n_groups(n_groups, None, batch_groups), max_gap, min_duration,
                                         min_count)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        out = C.POINTER(_abi.EpisodesResultC)()
        self._check(self.lib.mdb_episodes_list(self.handle, pointers, group_pointers, len(views), C.byref(request),
                                               C.byref(out)))
        try:
            result = out.contents
            n = int(result.n)
            if n == 0:
                episodes = np.zeros(0, dtype=EPISODE_DTYPE)
            else:
                buffer = (C.c_char * (n * EPISODE_DTYPE.itemsize)).from_address(result.episodes)
                episodes = np.frombuffer(buffer, dtype=EPISODE_DTYPE).copy()
            return episodes, int(result.n_rows), int(result.n_passing)
        finally:
            self.lib.mdb_episodes_result_free(out)

    def episodes_count_dev(self, dev_segments, flt, groups_ptr=None, n_groups=1, max_gap=None, min_duration=0,
                           min_count=0):
        """mdb_episodes_count_dev on a resident batch (groups_ptr: a device array or None): (n_episodes, n_rows,
        n_passing)."""
        request = self._episodes_request(flt, n_groups, max_gap, min_duration, min_count)
        n, n_rows, n_passing = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.mdb_episodes_count_dev(self.handle, C.byref(dev_segments.seg), C.c_void_p(groups_ptr),
                                                    C.byref(request), C.byref(n), C.byref(n_rows), C.byref(n_passing)))
        return n.value, n_rows.value, n_passing.value

    def episodes_into_dev(self, dev_segments, flt, out_ptr, cap, groups_ptr=None, n_groups=1, max_gap=None,
                          min_duration=0, min_count=0):
        """mdb_episodes_dev into `cap` device episodes at out_ptr: (n_out, n_rows, n_passing)."""
        request = self._episodes_request(flt, n_groups, max_gap, min_duration, min_count)
        n, n_rows, n_passing = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.mdb_episodes_dev(self.handle, C.byref(dev_segments.seg), C.c_void_p(groups_ptr),
                                              C.byref(request), C.c_void_p(out_ptr), int(cap), C.byref(n),
                                              C.byref(n_rows), C.byref(n_passing)))
        return n.value, n_rows.value, n_passing.value

    def episodes_dev(self, dev_segments, flt, groups=None, n_groups=None, max_gap=None, min_duration=0, min_count=0):
        """episodes() on a resident batch: `groups` is uploaded, the episodes are counted, written on the device
        (mdb_episodes_count_dev, mdb_episodes_dev) and downloaded."""
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, None, [groups])
        dev_groups = None if groups is None else self.upload_array(groups)
        out = None
        try:
            n, _, _ = self.episodes_count_dev(dev_segments, flt, dev_groups, n_groups, max_gap, min_duration, min_count)
            out = self.dev_alloc(EPISODE_DTYPE.itemsize * max(n, 1))
            produced, n_rows, n_passing = self.episodes_into_dev(dev_segments, flt, out, n, dev_groups, n_groups, max_gap,
                                                                 min_duration, min_count)
            assert produced == n
            episodes = self.download_array(out, n, EPISODE_DTYPE) if n else np.zeros(0, dtype=EPISODE_DTYPE)
            return episodes, n_rows, n_passing
        finally:
            if out is not None:
                self.dev_free(out)
            if dev_groups is not None:
                self.dev_free(dev_groups)

    # ---- moments of one field per value cell of another: count, mean and m2 of y per cell of x ----------

    @staticmethod
    def _binned_cells(cells, n_groups, n_buckets, n_cells):
        if cells is None:
            return fresh_moments_cells((n_groups, n_buckets, n_cells))
        if (cells.dtype != MOMENTS_CELL_DTYPE or cells.shape != (n_groups, n_buckets, n_cells)
                or not cells.flags.c_contiguous):
            raise ValueError(f"cells must be a contiguous ({n_groups}, {n_buckets}, {n_cells}) array of MOMENTS_CELL_DTYPE")
        return cells

    def binned_buckets(self, x, y, edges, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, cells=None,
                       n_groups=None):
        """The count, mean and m2 of the y values per bucket of date_bin(width, ts, origin), group and value cell of x
        (mdb_binned_buckets): x and y are two field batches of the same series that line up row for row, the cell of
        a pair is hist_cell_of(edges, its x value). Returns `cells` (or fresh ones), MOMENTS_CELL_DTYPE of shape
        (n_groups, n_buckets, len(edges) + 1), merged in place: moments_merge and moments_variance apply. `groups` (per
        segment of x) and n_groups as for agg_buckets. `x is y` is uploaded once."""
        edges = _edges_array(edges)
        groups = self._groups_array(groups, len(x))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._binned_cells(cells, n_groups, n_buckets, len(edges) + 1)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        x_view = x.as_c()
        y_view = x_view if y is x else y.as_c()
        self._check(self.lib.mdb_binned_buckets(self.handle, C.byref(x_view), C.byref(y_view),
                                                None if groups is None else groups.ctypes.data_as(C.c_void_p),
                                                C.byref(request), edges.ctypes.data_as(C.c_void_p), len(edges),
                                                cells.ctypes.data_as(C.c_void_p)))
        return cells

    def binned_buckets_list(self, xs, ys, edges, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                            cells=None, n_groups=None):
        """Several host batches per field merged as one (mdb_binned_buckets_list): the cuts of xs and ys need not
        coincide; `groups`: None or one array (or None) per batch of xs."""
        edges = _edges_array(edges)
        batch_groups = [None] * len(xs) if groups is None else [self._groups_array(g, len(b))
                                                                for g, b in zip(groups, xs)]
        n_groups = self._n_groups(n_groups, cells, batch_groups)
        cells = self._binned_cells(cells, n_groups, n_buckets, len(edges) + 1)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        x_views = [batch.as_c() for batch in xs]
        y_views = [batch.as_c() for batch in ys]
        x_pointers = (C.POINTER(_abi.SegmentsC) * max(len(x_views), 1))(*[C.pointer(view) for view in x_views])
        y_pointers = (C.POINTER(_abi.SegmentsC) * max(len(y_views), 1))(*[C.pointer(view) for view in y_views])
        group_pointers = (C.c_void_p * max(len(x_views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_binned_buckets_list(self.handle, x_pointers, len(x_views), y_pointers, len(y_views),
                                                     group_pointers, C.byref(request),
                                                     edges.ctypes.data_as(C.c_void_p), len(edges),
                                                     cells.ctypes.data_as(C.c_void_p)))
        return cells

    def binned_buckets_dev(self, dev_x, dev_y, edges, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                           cells=None, n_groups=None):
        """mdb_binned_buckets_dev on two resident batches: `groups` and `cells` are uploaded, the cells downloaded
        again."""
        edges = _edges_array(edges)
        groups = self._groups_array(groups, len(dev_x))
        n_groups = self._n_groups(n_groups, cells, [groups])
        cells = self._binned_cells(cells, n_groups, n_buckets, len(edges) + 1)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_cells = self.upload_array(cells)
        try:
            self._check(self.lib.mdb_binned_buckets_dev(self.handle, C.byref(dev_x.seg), C.byref(dev_y.seg),
                                                        None if dev_groups is None else C.c_void_p(dev_groups),
                                                        C.byref(request), edges.ctypes.data_as(C.c_void_p), len(edges),
                                                        C.c_void_p(dev_cells)))
            cells[...] = self.download_array(dev_cells, cells.size, MOMENTS_CELL_DTYPE).reshape(cells.shape)
        finally:
            self.dev_free(dev_cells)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return cells

    def binned(self, x, y, edges, t_lo=None, t_hi=None, groups=None, n_groups=None):
        """The cells of the pairs of `x` and `y` inside [t_lo, t_hi] per group and value cell of x, shape
        (n_groups, len(edges) + 1): one bucket over the data inside the range - the power curve."""
        n_cells = len(_edges_array(edges)) + 1
        n_groups = self._n_groups(n_groups, None, [self._groups_array(groups, len(x))])
        if len(x) == 0:
            return fresh_moments_cells((n_groups, n_cells))
        lo, hi = int(np.min(x.start_time)), int(np.max(x.end_time))
        lo = lo if t_lo is None else max(lo, int(t_lo))
        hi = hi if t_hi is None else min(hi, int(t_hi))
        if lo > hi:
            return fresh_moments_cells((n_groups, n_cells))
        if hi - lo + 1 > INT64_MAX:
            raise ValueError("the data inside the range spans more than one bucket can hold: use binned_buckets")
        return self.binned_buckets(x, y, edges, lo, hi - lo + 1, 1, groups, lo, hi, None, n_groups).reshape(n_groups, n_cells)

    @staticmethod
    def _n_groups(n_groups, states, groups):
        if n_groups is not None:
            return int(n_groups)
        if states is not None:
            return int(states.shape[0])
        return max([int(g.max()) + 1 for g in groups if g is not None and g.size] or [1])

    # ---- value histograms and quantiles ------------------------------------------------------------

    @staticmethod
    def _hist_request(edges, n_groups, t_lo, t_hi):
        return _abi.HistRequestC(INT64_MIN if t_lo is None else int(t_lo), INT64_MAX if t_hi is None else int(t_hi),
                                 len(edges), int(n_groups), 0, 0)

    @staticmethod
    def _hist_counts(counts, n_groups, n_cells):
        if counts is None:
            return np.zeros((n_groups, n_cells), dtype=np.uint64)
        if counts.dtype != np.uint64 or counts.shape != (n_groups, n_cells) or not counts.flags.c_contiguous:
            raise ValueError(f"counts must be a contiguous ({n_groups}, {n_cells}) array of uint64")
        return counts

    def hist(self, batch, edges, groups=None, t_lo=None, t_hi=None, counts=None, n_groups=None):
        """The points of `batch` inside [t_lo, t_hi] ADDED to `counts` (or to fresh zeros), shape (n_groups,
        len(edges) + 1): cell c of a value = the number of edges at or below it in totalOrder (mdb_hist_batch).
        `groups`: one id per segment row (None: all in group 0); n_groups defaults to counts' rows, else to
        max(groups) + 1."""
        return self.hist_list([batch], edges, None if groups is None else [groups], t_lo, t_hi, counts, n_groups)

    def hist_list(self, batches, edges, groups=None, t_lo=None, t_hi=None, counts=None, n_groups=None):
        """Several host batches counted as one (mdb_hist_batch_list); `groups`: None or one array (or None) per batch."""
        edges = _edges_array(edges)
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, counts, batch_groups)
        counts = self._hist_counts(counts, n_groups, len(edges) + 1)
        request = self._hist_request(edges, n_groups, t_lo, t_hi)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_hist_batch_list(self.handle, pointers, group_pointers, len(views), C.byref(request),
                                                 edges.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
        return counts

    def hist_dev(self, dev_segments, edges, groups=None, t_lo=None, t_hi=None, counts=None, n_groups=None):
        """mdb_hist_batch_dev on a resident batch: `groups` and `counts` are uploaded, the counts downloaded again."""
        edges = _edges_array(edges)
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, counts, [groups])
        counts = self._hist_counts(counts, n_groups, len(edges) + 1)
        request = self._hist_request(edges, n_groups, t_lo, t_hi)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_counts = self.upload_array(counts)
        try:
            self._check(self.lib.mdb_hist_batch_dev(self.handle, C.byref(dev_segments.seg),
                                                    None if dev_groups is None else C.c_void_p(dev_groups),
                                                    C.byref(request), edges.ctypes.data_as(C.c_void_p),
                                                    C.c_void_p(dev_counts)))
            counts[...] = self.download_array(dev_counts, counts.size, np.uint64).reshape(counts.shape)
        finally:
            self.dev_free(dev_counts)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return counts

    def _quantile(self, call, seg, q, t_lo, t_hi, interpolate):
        q = np.atleast_1d(np.ascontiguousarray(q, dtype=np.float64))
        lo = np.full(len(q), np.nan, dtype=np.float32)
        hi = np.full(len(q), np.nan, dtype=np.float32)
        n_points = C.c_uint64()
        self._check(call(self.handle, C.byref(seg), INT64_MIN if t_lo is None else int(t_lo),
                         INT64_MAX if t_hi is None else int(t_hi), q.ctypes.data_as(C.c_void_p), len(q),
                         lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), C.byref(n_points)))
        if not interpolate:
            return lo, hi, n_points.value
        if n_points.value == 0:
            return np.full(len(q), np.nan), 0
        fractions = np.array([quantile_positions(x, n_points.value)[2] for x in q])
        wide_lo, wide_hi = lo.astype(np.float64), hi.astype(np.float64)
        with np.errstate(invalid="ignore"):
            # (equal ends - also infinite ones - are the value itself: no inf - inf)
            values = np.where(lo.view(np.uint32) == hi.view(np.uint32), wide_lo, wide_lo + (wide_hi - wide_lo) * fractions)
        return values, n_points.value

    def quantile(self, batch, q, t_lo=None, t_hi=None, interpolate=False):
        """Exact order statistics of the points of `batch` inside [t_lo, t_hi], in totalOrder (mdb_quantile_batch):
        (lo, hi, n_points) with lo[i] / hi[i] the floor / ceil ranks of q[i] * (n_points - 1) (NaN-filled when there
        is no point); interpolate=True: (lo + (hi - lo) * fraction in f64 - DataFusion's percentile_cont, and its
        median for q = 0.5 - and n_points)."""
        return self._quantile(self.lib.mdb_quantile_batch, batch.as_c(), q, t_lo, t_hi, interpolate)

    def quantile_dev(self, dev_segments, q, t_lo=None, t_hi=None, interpolate=False):
        """quantile on a resident batch (mdb_quantile_batch_dev)."""
        return self._quantile(self.lib.mdb_quantile_batch_dev, dev_segments.seg, q, t_lo, t_hi, interpolate)

    # ---- value histograms and quantiles per time bucket ---------------------------------------------

    @staticmethod
    def _hist_bucket_counts(counts, n_groups, n_buckets, n_cells):
        if counts is None:
            return np.zeros((n_groups, n_buckets, n_cells), dtype=np.uint64)
        if counts.dtype != np.uint64 or counts.shape != (n_groups, n_buckets, n_cells) or not counts.flags.c_contiguous:
            raise ValueError(f"counts must be a contiguous ({n_groups}, {n_buckets}, {n_cells}) array of uint64")
        return counts

    def hist_buckets(self, batch, edges, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, counts=None,
                     n_groups=None):
        """The points of `batch` ADDED to `counts` (or to fresh zeros), shape (n_groups, n_buckets, len(edges) + 1): per
        bucket of date_bin(width, ts, origin) and group the histogram `hist` gives for one range (mdb_hist_buckets).
        `groups` and n_groups as for agg_buckets."""
        return self.hist_buckets_list([batch], edges, origin, width, n_buckets, None if groups is None else [groups],
                                      t_lo, t_hi, counts, n_groups)

    def hist_buckets_list(self, batches, edges, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                          counts=None, n_groups=None):
        """Several host batches counted as one (mdb_hist_buckets_list); `groups`: None or one array (or None) per
        batch."""
        edges = _edges_array(edges)
        batch_groups = [None] * len(batches) if groups is None else [self._groups_array(g, len(b))
                                                                     for g, b in zip(groups, batches)]
        n_groups = self._n_groups(n_groups, counts, batch_groups)
        counts = self._hist_bucket_counts(counts, n_groups, n_buckets, len(edges) + 1)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        views = [batch.as_c() for batch in batches]
        pointers = (C.POINTER(_abi.SegmentsC) * max(len(views), 1))(*[C.pointer(view) for view in views])
        group_pointers = (C.c_void_p * max(len(views), 1))(
            *[None if g is None else g.ctypes.data_as(C.c_void_p).value for g in batch_groups])
        self._check(self.lib.mdb_hist_buckets_list(self.handle, pointers, group_pointers, len(views), C.byref(request),
                                                   edges.ctypes.data_as(C.c_void_p), len(edges),
                                                   counts.ctypes.data_as(C.c_void_p)))
        return counts

    def hist_buckets_dev(self, dev_segments, edges, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                         counts=None, n_groups=None):
        """mdb_hist_buckets_dev on a resident batch: `groups` and `counts` are uploaded, the counts downloaded again."""
        edges = _edges_array(edges)
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, counts, [groups])
        counts = self._hist_bucket_counts(counts, n_groups, n_buckets, len(edges) + 1)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        dev_groups = None if groups is None else self.upload_array(groups)
        dev_counts = self.upload_array(counts)
        try:
            self._check(self.lib.mdb_hist_buckets_dev(self.handle, C.byref(dev_segments.seg),
                                                      None if dev_groups is None else C.c_void_p(dev_groups),
                                                      C.byref(request), edges.ctypes.data_as(C.c_void_p), len(edges),
                                                      C.c_void_p(dev_counts)))
            counts[...] = self.download_array(dev_counts, counts.size, np.uint64).reshape(counts.shape)
        finally:
            self.dev_free(dev_counts)
            if dev_groups is not None:
                self.dev_free(dev_groups)
        return counts

    def _quantile_buckets(self, call, seg, groups, q, origin, width, n_buckets, n_groups, t_lo, t_hi, interpolate):
        q = np.atleast_1d(np.ascontiguousarray(q, dtype=np.float64))
        shape = (n_groups, n_buckets, len(q))
        lo = np.full(shape, np.nan, dtype=np.float32)
        hi = np.full(shape, np.nan, dtype=np.float32)
        n_points = np.zeros((n_groups, n_buckets), dtype=np.uint64)
        request = self._bucket_request(origin, width, n_buckets, n_groups, t_lo, t_hi, 0)
        self._check(call(self.handle, C.byref(seg), groups, C.byref(request), q.ctypes.data_as(C.c_void_p), len(q),
                         lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
                         n_points.ctypes.data_as(C.c_void_p)))
        if not interpolate:
            return lo, hi, n_points
        last = np.maximum(n_points, 1).astype(np.float64) - 1.0
        positions = q[None, None, :] * last[:, :, None]  # (p = q * (double)(N - 1), as mdb_quantile_positions)
        fractions = positions - np.floor(positions)
        wide_lo, wide_hi = lo.astype(np.float64), hi.astype(np.float64)
        with np.errstate(invalid="ignore"):
            # (equal ends - also infinite ones - are the value itself: no inf - inf; a cell without a point stays NaN)
            values = np.where(lo.view(np.uint32) == hi.view(np.uint32), wide_lo, wide_lo + (wide_hi - wide_lo) * fractions)
        return values, n_points

    def quantile_buckets(self, batch, q, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None, n_groups=None,
                         interpolate=False):
        """Exact order statistics per bucket of date_bin(width, ts, origin) and group (mdb_quantile_buckets): (lo, hi,
        n_points) with lo / hi of shape (n_groups, n_buckets, len(q)) - the floor / ceil ranks of q[i] * (N - 1) among
        the cell's N points, NaN-filled where N == 0 - and n_points of shape (n_groups, n_buckets). interpolate=True:
        (lo + (hi - lo) * fraction in f64, n_points), as `quantile`. At most MDB_QUANTILE_BUCKETS_MAX_Q quantiles."""
        groups = self._groups_array(groups, len(batch))
        n_groups = self._n_groups(n_groups, None, [groups])
        pointer = None if groups is None else groups.ctypes.data_as(C.c_void_p)
        return self._quantile_buckets(self.lib.mdb_quantile_buckets, batch.as_c(), pointer, q, origin, width, n_buckets,
                                      n_groups, t_lo, t_hi, interpolate)

    def quantile_buckets_dev(self, dev_segments, q, origin, width, n_buckets, groups=None, t_lo=None, t_hi=None,
                             n_groups=None, interpolate=False):
        """quantile_buckets on a resident batch (mdb_quantile_buckets_dev): `groups` is uploaded."""
        groups = self._groups_array(groups, len(dev_segments))
        n_groups = self._n_groups(n_groups, None, [groups])
        dev_groups = None if groups is None else self.upload_array(groups)
        try:
            return self._quantile_buckets(self.lib.mdb_quantile_buckets_dev, dev_segments.seg,
                                          None if dev_groups is None else C.c_void_p(dev_groups), q, origin, width,
                                          n_buckets, n_groups, t_lo, t_hi, interpolate)
        finally:
            if dev_groups is not None:
                self.dev_free(dev_groups)

    # ---- fit -------------------------------------------------------------------------------------

    def compress_chunks(self, timestamps, values, chunk_offsets, eb):
        ts = np.ascontiguousarray(timestamps, dtype=np.int64)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if len(ts) != len(v):
            # compression.rs:202-206
            raise HipError(
                "Uncompressed timestamps and uncompressed values have different lengths.")
        offsets = np.ascontiguousarray(chunk_offsets, dtype=np.uint64)
        out = C.POINTER(_abi.SegmentsOwnedC)()
        started = time.perf_counter()
        code = self.lib.mdb_compress_chunks(
            self.handle, ts.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
            offsets.ctypes.data_as(C.c_void_p), len(offsets) - 1, eb, C.byref(out))
        self.last_call_seconds = time.perf_counter() - started
        self._check(code)
        try:
            return SegmentBatch.from_owned(out)
        finally:
            self.lib.mdb_segments_free(out)

    def compress_chunk_list(self, chunks, eb):
        """mdb_compress_chunk_list: chunks = [(timestamps, values), ...] lying wherever they lie."""
        arrays = [(np.ascontiguousarray(ts, dtype=np.int64), np.ascontiguousarray(v, dtype=np.float32))
                  for ts, v in chunks]
        for ts, v in arrays:
            if len(ts) != len(v):
                raise HipError("Uncompressed timestamps and uncompressed values have different lengths.")
        # (an array that was contiguous already is passed as it is: chunks that share a timestamp array
        # keep sharing it)
        table = (_abi.ChunkC * max(len(arrays), 1))(*[_abi.ChunkC(ts.ctypes.data, v.ctypes.data, len(v))
                                                      for ts, v in arrays])
        out = C.POINTER(_abi.SegmentsOwnedC)()
        started = time.perf_counter()
        code = self.lib.mdb_compress_chunk_list(self.handle, table, len(arrays), eb, C.byref(out))
        self.last_call_seconds = time.perf_counter() - started  # (the library call alone, for bench.py)
        self._check(code)
        try:
            return SegmentBatch.from_owned(out)
        finally:
            self.lib.mdb_segments_free(out)

    def try_compress_univariate_time_series(self, timestamps, values, eb):
        """compression.rs:191-275 for one sorted series."""
        return self.compress_chunks(timestamps, values, [0, len(values)], eb)

    def compress_chunks_dev(self, ts_ptr, values_ptr, chunk_offsets_ptr, n_chunks, eb,
                            regular_start=0, regular_interval=0, series_first_index_ptr=None):
        out = C.POINTER(_abi.SegmentsOwnedC)()
        self._check(self.lib.mdb_compress_chunks_dev(
            self.handle, C.c_void_p(ts_ptr), C.c_void_p(values_ptr), C.c_void_p(chunk_offsets_ptr),
            n_chunks, eb, regular_start, regular_interval, C.c_void_p(series_first_index_ptr),
            C.byref(out)))
        return DeviceSegments(self, out)

    def try_split_and_compress_univariate_time_series(self, timestamps, field_values, error_bounds):
        """compression.rs:147-179: one sorted series, several field columns sharing its timestamps,
        one error bound per field. Returns one SegmentBatch per field."""
        ts = np.ascontiguousarray(timestamps, dtype=np.int64)
        fields = [np.ascontiguousarray(v, dtype=np.float32) for v in field_values]
        for v in fields:
            if len(v) != len(ts):
                raise HipError(
                    "Uncompressed timestamps and uncompressed values have different lengths.")
        n_fields = len(fields)
        pointers = (C.c_void_p * max(n_fields, 1))(*[v.ctypes.data for v in fields])
        bounds = (_abi.ErrorBoundC * max(n_fields, 1))(*error_bounds)
        out = (C.POINTER(_abi.SegmentsOwnedC) * max(n_fields, 1))()
        self._check(self.lib.mdb_split_and_compress_univariate(
            self.handle, ts.ctypes.data_as(C.c_void_p), pointers, bounds, n_fields, len(ts), out))
        batches = []
        for f in range(n_fields):
            try:
                batches.append(SegmentBatch.from_owned(out[f]))
            finally:
                self.lib.mdb_segments_free(out[f])
        return batches

    def validate_segments_dev(self, dev_segments):
        """Raises HipError if an out-of-line view of a device batch points outside its buffers."""
        seg = dev_segments.seg if hasattr(dev_segments, "seg") else dev_segments
        self._check(self.lib.mdb_segments_validate_dev(self.handle, C.byref(seg)))

    # ---- multi-GPU: the final aggregate merge over RCCL ------------------------------------------

    def comm_init(self, rank, world, unique_id):
        """ncclCommInitRank on this context's device (collective). `unique_id`: the 128 bytes of
        `comm_unique_id()` made by ONE rank and handed to the others."""
        buffer = C.create_string_buffer(bytes(unique_id), _abi.MDB_COMM_ID_BYTES)
        self._check(self.lib.mdb_comm_init(self.handle, rank, world, buffer))

    def comm_close(self):
        self._check(self.lib.mdb_comm_close(self.handle))

    def agg_all_reduce(self, state):
        """Merge the partial aggregate states of all ranks (one 32-byte all-gather over RCCL + a
        rank-ordered fold). Returns (merged state, ranks seen)."""
        merged = _abi.AggStateC(state.sum, state.count, state.min, state.max)
        seen = C.c_int32()
        self._check(self.lib.mdb_agg_all_reduce(self.handle, C.byref(merged), C.byref(seen)))
        return merged, seen.value

    def synth_values_dev(self, out_ptr, first_series, n_series, n_per_series,
                         seed=0x4D44425F52454631):
        self._check(self.lib.mdb_synth_values_dev(self.handle, C.c_void_p(out_ptr), first_series,
                                                  n_series, n_per_series, seed))

    # ---- measurement -----------------------------------------------------------------------------

    def profile_enable(self, enabled=True):
        self._check(self.lib.mdb_profile_enable(self.handle, int(enabled)))

    def profile_reset(self):
        self._check(self.lib.mdb_profile_reset(self.handle))

    def profile(self):
        """{kernel name: (launches, total_ms)} since the last reset."""
        names = C.create_string_buffer(4096)
        self._check(self.lib.mdb_profile_names(self.handle, names, 4096))
        out = {}
        for name in filter(None, names.value.decode().split("\n")):
            launches, total_ms = C.c_uint64(), C.c_double()
            self._check(self.lib.mdb_profile_get(self.handle, name.encode(), C.byref(launches),
                                                 C.byref(total_ms)))
            out[name] = (launches.value, total_ms.value)
        return out
