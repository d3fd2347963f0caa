"""ctypes mirror of include/mdb_format.h and include/mdb.h, plus the loader of libmdb_hip.so.

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded,
``load_hip_library`` raises. The structs here are shared with the oracle wrapper in ``tests/`` so
both sides consume exactly the same in-memory segment batches.
"""

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
# MDB_HIP_LIBRARY selects another build of the same library (A/B timing of kernel variants).
HIP_LIBRARY_PATH = os.environ.get("MDB_HIP_LIBRARY", os.path.join(_HERE, "csrc", "libmdb_hip.so"))

MDB_PMC_MEAN_ID = 0
MDB_SWING_ID = 1
MDB_MACAQUE_V_ID = 2
MODEL_TYPE_NAMES = ("pmc_mean", "swing", "macaque_v")  # models/mod.rs:44

MDB_EB_LOSSLESS = 0
MDB_EB_ABSOLUTE = 1
MDB_EB_RELATIVE = 2

MDB_AGG_COUNT = 1
MDB_AGG_MIN = 2
MDB_AGG_MAX = 4
MDB_AGG_SUM = 8
MDB_AGG_AVG = 16

MDB_COMM_ID_BYTES = 128

# mdb_value_filter flags (mdb_format.h)
MDB_VALUE_LO_OPEN = 1
MDB_VALUE_HI_OPEN = 2
MDB_VALUE_NO_LO = 4
MDB_VALUE_NO_HI = 8

# mdb_mask_combine_dev operations (mdb.h)
MDB_MASK_AND = 0
MDB_MASK_OR = 1
MDB_MASK_XOR = 2
MDB_MASK_ANDNOT = 3
MDB_MASK_NOT = 4

MDB_GRID_HAS_RANGE = 1
MDB_GRID_VALUES_ONLY = 2

F32_MAX = 3.4028234663852886e38


class ErrorBoundC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("value", C.c_float)]


class BinViewColC(C.Structure):
    _fields_ = [
        ("views", C.c_void_p),
        ("buffers", C.POINTER(C.c_void_p)),
        ("buffer_sizes", C.POINTER(C.c_int64)),
        ("n_buffers", C.c_int32),
    ]


class SegmentsC(C.Structure):
    _fields_ = [
        ("n", C.c_uint64),
        ("model_type_id", C.c_void_p),
        ("start_time", C.c_void_p),
        ("end_time", C.c_void_p),
        ("timestamps", BinViewColC),
        ("min_value", C.c_void_p),
        ("max_value", C.c_void_p),
        ("values", BinViewColC),
        ("residuals", BinViewColC),
    ]


class GridMetricsC(C.Structure):
    _fields_ = [
        ("rows_created", C.c_uint64),
        ("rows_created_by_model_type", C.c_uint64 * 3),
        ("segments_with_residuals", C.c_uint64),
        ("segments_with_model_type", C.c_uint64 * 3),
        ("segments_regular", C.c_uint64),
        ("segments_irregular", C.c_uint64),
    ]

    def as_dict(self):
        out = {"rows_created": self.rows_created}
        for i, name in enumerate(MODEL_TYPE_NAMES):
            out[f"rows_created_by_{name}"] = self.rows_created_by_model_type[i]
        out["segments_with_residuals"] = self.segments_with_residuals
        for i, name in enumerate(MODEL_TYPE_NAMES):
            out[f"segments_with_{name}"] = self.segments_with_model_type[i]
        out["regular_segments"] = self.segments_regular
        out["irregular_segments"] = self.segments_irregular
        return out


class AggStateC(C.Structure):
    _fields_ = [
        ("sum", C.c_double),
        ("count", C.c_int64),
        ("min", C.c_float),
        ("max", C.c_float),
    ]

    @classmethod
    def fresh(cls):
        # model_simple_aggregates.rs:413,456: min starts at f32::MAX, max at f32::MIN.
        return cls(0.0, 0, F32_MAX, -F32_MAX)


class SegmentsOwnedC(C.Structure):
    _fields_ = [
        ("seg", SegmentsC),
        ("error", C.c_void_p),
        ("chunk_index", C.c_void_p),
        ("on_device", C.c_int32),
        ("priv_", C.c_void_p),
    ]


class GridResultC(C.Structure):
    _fields_ = [
        ("timestamps", C.c_void_p),
        ("values", C.c_void_p),
        ("rows_per_segment", C.c_void_p),
        ("n", C.c_uint64),
        ("n_segments", C.c_uint64),
        ("reserved_front", C.c_uint64),
        ("metrics", GridMetricsC),
        ("priv_", C.c_void_p),
    ]


class GridInputC(C.Structure):
    _fields_ = [
        ("segments", SegmentsC),
        ("tag_views", C.POINTER(C.c_void_p)),
        ("tag_buffer_shift", C.POINTER(C.c_int32)),
    ]


class GridRequestC(C.Structure):
    _fields_ = [
        ("flags", C.c_uint32),
        ("n_tag_columns", C.c_uint32),
        ("t_lo", C.c_int64),
        ("t_hi", C.c_int64),
        ("reserve_front", C.c_uint64),
    ]


class ChunkC(C.Structure):
    _fields_ = [("ts", C.c_void_p), ("values", C.c_void_p), ("n", C.c_uint64)]


class BucketRequestC(C.Structure):
    """mdb_bucket_request: the buckets of date_bin(width, ts, origin) for mdb_agg_buckets*."""
    _fields_ = [
        ("origin", C.c_int64),
        ("width", C.c_int64),
        ("n_buckets", C.c_uint64),
        ("t_lo", C.c_int64),
        ("t_hi", C.c_int64),
        ("n_groups", C.c_uint32),
        ("which_mask", C.c_uint32),
    ]


class ValueFilterC(C.Structure):
    """mdb_value_filter: a time range ANDed with value bounds compared in IEEE totalOrder (MDB_VALUE_* flags)."""
    _fields_ = [
        ("t_lo", C.c_int64),
        ("t_hi", C.c_int64),
        ("v_lo", C.c_float),
        ("v_hi", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class EpisodeC(C.Structure):
    """mdb_episode: one maximal run of passing rows (mdb_episodes*)."""
    _fields_ = [
        ("first_row", C.c_uint64),
        ("count", C.c_uint64),
        ("t_first", C.c_int64),
        ("t_last", C.c_int64),
        ("sum", C.c_double),
        ("min", C.c_float),
        ("max", C.c_float),
        ("group", C.c_uint32),
        ("first_segment", C.c_uint32),
        ("reserved", C.c_uint64),
    ]


class EpisodesRequestC(C.Structure):
    """mdb_episodes_request: the value filter, the gap rule and the minimum filters of mdb_episodes*."""
    _fields_ = [
        ("filter", ValueFilterC),
        ("max_gap", C.c_int64),
        ("min_duration", C.c_int64),
        ("min_count", C.c_uint64),
        ("n_groups", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class EpisodesResultC(C.Structure):
    _fields_ = [
        ("episodes", C.c_void_p),
        ("n", C.c_uint64),
        ("n_rows", C.c_uint64),
        ("n_passing", C.c_uint64),
        ("priv_", C.c_void_p),
    ]


assert C.sizeof(EpisodeC) == 64 and C.sizeof(EpisodesRequestC) == 64

MDB_INTEGRAL_LINEAR = 0
MDB_INTEGRAL_STEP = 1


class IntegralCellC(C.Structure):
    """mdb_integral_cell: the defined time of a bucket and the integral of the series over it (mdb_integral_buckets*)."""
    _fields_ = [("duration", C.c_uint64), ("integral", C.c_double)]


class IntegralRequestC(C.Structure):
    """mdb_integral_request: the buckets (no time range, which_mask 0), the gap rule and the interpolation."""
    _fields_ = [
        ("buckets", BucketRequestC),
        ("max_gap", C.c_int64),
        ("method", C.c_uint32),
        ("flags", C.c_uint32),
    ]


assert C.sizeof(IntegralCellC) == 16 and C.sizeof(IntegralRequestC) == 64

MDB_SAMPLE_LINEAR = 0
MDB_SAMPLE_STEP = 1
MDB_SAMPLE_EXACT = 2


class SampleCellC(C.Structure):
    """mdb_sample_cell: the contributions an instant received and their f64 sum (mdb_sample_at*)."""
    _fields_ = [("count", C.c_uint64), ("sum", C.c_double)]


class SampleRequestC(C.Structure):
    """mdb_sample_request: the instants (no time range, which_mask 0), the gap rule and the method."""
    _fields_ = [
        ("instants", BucketRequestC),
        ("max_gap", C.c_int64),
        ("method", C.c_uint32),
        ("flags", C.c_uint32),
    ]


assert C.sizeof(SampleCellC) == 16 and C.sizeof(SampleRequestC) == 64

MDB_CHANGE_NET = 0
MDB_CHANGE_VARIATION = 1
MDB_CHANGE_INCREASE = 2
MDB_CHANGE_RATE = 3


class ChangeCellC(C.Structure):
    """mdb_change_cell: the linked pairs whose later row lies in a bucket (mdb_change_buckets*)."""
    _fields_ = [
        ("count", C.c_uint64),
        ("n_fall", C.c_uint64),
        ("duration", C.c_uint64),
        ("rise", C.c_double),
        ("fall", C.c_double),
        ("reset_sum", C.c_double),
        ("max_rise", C.c_double),
        ("max_fall", C.c_double),
    ]


class ChangeRequestC(C.Structure):
    """mdb_change_request: the buckets (no time range, which_mask 0) and the gap rule."""
    _fields_ = [
        ("buckets", BucketRequestC),
        ("max_gap", C.c_int64),
        ("reserved", C.c_uint32),
        ("flags", C.c_uint32),
    ]


assert C.sizeof(ChangeCellC) == 64 and C.sizeof(ChangeRequestC) == 64
assert [getattr(ChangeCellC, name).offset for name, _ in ChangeCellC._fields_] == [0, 8, 16, 24, 32, 40, 48, 56]

MDB_DWELL_STEP = 1


class DwellRequestC(C.Structure):
    """mdb_dwell_request: the buckets (no time range, which_mask 0), the gap rule and the method (MDB_DWELL_STEP)."""
    _fields_ = [
        ("buckets", BucketRequestC),
        ("max_gap", C.c_int64),
        ("method", C.c_uint32),
        ("flags", C.c_uint32),
    ]


assert C.sizeof(DwellRequestC) == 64


class TransitRequestC(C.Structure):
    """mdb_transit_request: the buckets (no time range, which_mask 0) and the gap rule; reserved and flags are 0."""
    _fields_ = [
        ("buckets", BucketRequestC),
        ("max_gap", C.c_int64),
        ("reserved", C.c_uint32),
        ("flags", C.c_uint32),
    ]


assert C.sizeof(TransitRequestC) == 64


class M4CellC(C.Structure):
    """mdb_m4_cell: the first, last, lowest and highest point of one bucket and group (mdb_m4_buckets*)."""
    _fields_ = [
        ("count", C.c_int64),
        ("t_first", C.c_int64),
        ("t_last", C.c_int64),
        ("t_min", C.c_int64),
        ("t_max", C.c_int64),
        ("v_first", C.c_float),
        ("v_last", C.c_float),
        ("v_min", C.c_float),
        ("v_max", C.c_float),
    ]


class MomentsCellC(C.Structure):
    """mdb_moments_cell: the count, the mean and m2 = sum((v - mean)^2) of one bucket and group (mdb_moments_buckets*)."""
    _fields_ = [
        ("count", C.c_int64),
        ("mean", C.c_double),
        ("m2", C.c_double),
    ]


class ComomentsCellC(C.Structure):
    """mdb_comoments_cell: the count, both means, both m2 and c_xy = sum((x - mean_x) * (y - mean_y)) of the pairs of
    one bucket and group (mdb_comoments_buckets*)."""
    _fields_ = [
        ("count", C.c_int64),
        ("mean_x", C.c_double),
        ("mean_y", C.c_double),
        ("m2_x", C.c_double),
        ("m2_y", C.c_double),
        ("c_xy", C.c_double),
    ]


MDB_DERIVED_LINEAR = 0
MDB_DERIVED_PRODUCT = 1
MDB_DERIVED_RATIO = 2
MDB_DERIVED_ABS = 1
MDB_DERIVED_SHORT_ROWS = 64     # an interval of at most this many rows is reduced by one lane
MDB_DERIVED_CHUNK_ROWS = 1024   # a longer one by one wave per chunk of this many rows


class DerivedExprC(C.Structure):
    """mdb_derived_expr: z = f(x, y) of mdb_derived_* - LINEAR ((a * x) + (b * y)) + c, PRODUCT (a * (x * y)) + c or
    RATIO (a * (x / y)) + c, with the optional ABS flag."""
    _fields_ = [
        ("op", C.c_uint32),
        ("flags", C.c_uint32),
        ("a", C.c_float),
        ("b", C.c_float),
        ("c", C.c_float),
    ]


class DerivedCellC(C.Structure):
    """mdb_derived_cell: the count, mean, m2, min and max of the generated values z of one bucket and group
    (mdb_derived_buckets*)."""
    _fields_ = [
        ("count", C.c_int64),
        ("mean", C.c_double),
        ("m2", C.c_double),
        ("min", C.c_float),
        ("max", C.c_float),
    ]


MDB_ROLL_AGG = 0         # mdb_agg_state, 24 B
MDB_ROLL_M4 = 1          # mdb_m4_cell, 56 B
MDB_ROLL_MOMENTS = 2     # mdb_moments_cell, 24 B (also binned)
MDB_ROLL_COMOMENTS = 3   # mdb_comoments_cell, 48 B (also trend)
MDB_ROLL_DERIVED = 4     # mdb_derived_cell, 32 B
MDB_ROLL_INTEGRAL = 5    # mdb_integral_cell, 16 B
MDB_ROLL_CHANGE = 6      # mdb_change_cell, 64 B
MDB_ROLL_U64 = 7         # uint64_t, wrapping add (hist_buckets, dwell, transit)


class RollRequestC(C.Structure):
    """mdb_roll_request: windows of `window` adjacent buckets every `stride` buckets over cells viewed as row-major
    [n_outer][n_buckets][n_inner] (mdb_roll_cells*)."""
    _fields_ = [
        ("kind", C.c_uint32),
        ("flags", C.c_uint32),
        ("n_outer", C.c_uint64),
        ("n_buckets", C.c_uint64),
        ("n_inner", C.c_uint64),
        ("window", C.c_uint64),
        ("stride", C.c_uint64),
    ]


class HistRequestC(C.Structure):
    """mdb_hist_request: the time range, number of edges and number of groups of mdb_hist_batch*."""
    _fields_ = [
        ("t_lo", C.c_int64),
        ("t_hi", C.c_int64),
        ("n_edges", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


MDB_HIST_MAX_EDGES = 4095
MDB_QUANTILE_BUCKETS_MAX_Q = 4
MDB_QUANTILE_BUCKETS_PASSES = 4

_HIP_SYMBOLS = {
    # name: (restype, argtypes)
    "mdb_init": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mdb_close": (C.c_int, [C.c_void_p]),
    "mdb_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mdb_last_error": (C.c_char_p, []),
    "mdb_version": (C.c_char_p, []),
    "mdb_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mdb_trim": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mdb_set_scratch_limit": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mdb_device_info": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_int32),
                                  C.POINTER(C.c_uint64)]),
    "mdb_dev_alloc": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mdb_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mdb_dev_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_dev_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_dev_sync": (C.c_int, [C.c_void_p]),
    "mdb_segments_upload": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC),
                                      C.POINTER(C.POINTER(SegmentsOwnedC))]),
    "mdb_segments_download": (C.c_int, [C.c_void_p, C.POINTER(SegmentsOwnedC),
                                        C.POINTER(C.POINTER(SegmentsOwnedC))]),
    "mdb_segments_free": (None, [C.POINTER(SegmentsOwnedC)]),
    "mdb_grid_count": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(C.c_uint64)]),
    "mdb_grid_batch": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                 C.POINTER(GridMetricsC)]),
    "mdb_grid_count_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(C.c_uint64)]),
    "mdb_grid_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(GridMetricsC)]),
    "mdb_grid_count_range": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64,
                                       C.POINTER(C.c_uint64)]),
    "mdb_grid_batch_range": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.POINTER(C.c_uint64), C.POINTER(GridMetricsC)]),
    "mdb_grid_count_range_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64,
                                           C.POINTER(C.c_uint64)]),
    "mdb_grid_batch_range_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.POINTER(C.c_uint64), C.POINTER(GridMetricsC)]),
    "mdb_grid_batch_owned": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_uint32, C.c_int64,
                                       C.c_int64, C.c_uint64, C.POINTER(C.POINTER(GridResultC))]),
    "mdb_grid_result_free": (None, [C.POINTER(GridResultC)]),
    "mdb_grid_submit": (C.c_int, [C.c_void_p, C.POINTER(GridInputC), C.c_uint32, C.POINTER(GridRequestC),
                                  C.POINTER(C.c_void_p)]),
    "mdb_grid_wait": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(GridResultC))]),
    "mdb_grid_cancel": (None, [C.c_void_p]),
    "mdb_grid_result_tag_views": (C.c_void_p, [C.POINTER(GridResultC), C.c_uint32]),
    "mdb_replicate_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_uint64]),
    "mdb_agg_batch": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_uint32,
                                C.POINTER(AggStateC)]),
    "mdb_agg_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_uint32,
                                    C.POINTER(AggStateC)]),
    "mdb_agg_batch_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.c_uint32, C.c_uint32,
                                     C.POINTER(AggStateC)]),
    "mdb_agg_batch_range": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64,
                                      C.c_uint32, C.POINTER(AggStateC)]),
    "mdb_agg_batch_range_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64,
                                          C.c_uint32, C.POINTER(AggStateC)]),
    "mdb_agg_batch_range_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.c_uint32, C.c_int64,
                                           C.c_int64, C.c_uint32, C.POINTER(AggStateC)]),
    "mdb_agg_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                  C.c_void_p]),
    "mdb_agg_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                      C.c_void_p]),
    "mdb_agg_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p),
                                       C.c_uint32, C.POINTER(BucketRequestC), C.c_void_p]),
    "mdb_m4_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC), C.c_void_p]),
    "mdb_m4_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                     C.c_void_p]),
    "mdb_m4_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p), C.c_uint32,
                                      C.POINTER(BucketRequestC), C.c_void_p]),
    "mdb_m4_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_moments_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                      C.c_void_p]),
    "mdb_moments_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                          C.c_void_p]),
    "mdb_moments_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p),
                                           C.c_uint32, C.POINTER(BucketRequestC), C.c_void_p]),
    "mdb_moments_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_moments_variance": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mdb_comoments_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(SegmentsC), C.c_void_p,
                                        C.POINTER(BucketRequestC), C.c_void_p]),
    "mdb_comoments_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(SegmentsC), C.c_void_p,
                                            C.POINTER(BucketRequestC), C.c_void_p]),
    "mdb_comoments_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.c_uint32,
                                             C.POINTER(C.POINTER(SegmentsC)), C.c_uint32, C.POINTER(C.c_void_p),
                                             C.POINTER(BucketRequestC), C.c_void_p]),
    "mdb_comoments_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_comoments_moments": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mdb_comoments_finish": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mdb_derived_values_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(SegmentsC), C.POINTER(DerivedExprC),
                                         C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64)]),
    "mdb_derived_values": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(SegmentsC), C.POINTER(DerivedExprC),
                                     C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mdb_derived_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(SegmentsC), C.c_void_p,
                                      C.POINTER(BucketRequestC), C.POINTER(DerivedExprC), C.c_void_p]),
    "mdb_derived_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(SegmentsC), C.c_void_p,
                                          C.POINTER(BucketRequestC), C.POINTER(DerivedExprC), C.c_void_p]),
    "mdb_derived_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.c_uint32,
                                           C.POINTER(C.POINTER(SegmentsC)), C.c_uint32, C.POINTER(C.c_void_p),
                                           C.POINTER(BucketRequestC), C.POINTER(DerivedExprC), C.c_void_p]),
    "mdb_derived_apply": (C.c_int, [C.POINTER(DerivedExprC), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mdb_derived_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_derived_stats": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "mdb_roll_windows": (C.c_int, [C.POINTER(RollRequestC), C.POINTER(C.c_uint64)]),
    "mdb_roll_cells": (C.c_int, [C.POINTER(RollRequestC), C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_roll_cells_dev": (C.c_int, [C.c_void_p, C.POINTER(RollRequestC), C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_trend_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                    C.c_void_p]),
    "mdb_trend_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                        C.c_void_p]),
    "mdb_trend_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p),
                                         C.c_uint32, C.POINTER(BucketRequestC), C.c_void_p]),
    "mdb_integral_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(IntegralRequestC),
                                       C.c_void_p]),
    "mdb_integral_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(IntegralRequestC),
                                           C.c_void_p]),
    "mdb_integral_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p),
                                            C.c_uint32, C.POINTER(IntegralRequestC), C.c_void_p]),
    "mdb_integral_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_integral_average": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "mdb_sample_at": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(SampleRequestC), C.c_void_p]),
    "mdb_sample_at_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(SampleRequestC),
                                    C.c_void_p]),
    "mdb_sample_at_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p), C.c_uint32,
                                     C.POINTER(SampleRequestC), C.c_void_p]),
    "mdb_sample_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_sample_values": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "mdb_change_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(ChangeRequestC),
                                     C.c_void_p]),
    "mdb_change_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(ChangeRequestC),
                                         C.c_void_p]),
    "mdb_change_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p),
                                          C.c_uint32, C.POINTER(ChangeRequestC), C.c_void_p]),
    "mdb_change_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_change_finish": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mdb_dwell_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(DwellRequestC), C.c_void_p,
                                    C.c_uint32, C.c_void_p]),
    "mdb_dwell_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(DwellRequestC),
                                        C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_dwell_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p), C.c_uint32,
                                         C.POINTER(DwellRequestC), C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_dwell_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_dwell_share": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mdb_transit_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(TransitRequestC),
                                      C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_transit_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(TransitRequestC),
                                          C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_transit_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p), C.c_uint32,
                                           C.POINTER(TransitRequestC), C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_transit_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_transit_crossings": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mdb_episodes_count_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(EpisodesRequestC),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mdb_episodes_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(EpisodesRequestC), C.c_void_p,
                                   C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mdb_episodes": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(EpisodesRequestC),
                               C.POINTER(C.POINTER(EpisodesResultC))]),
    "mdb_episodes_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p), C.c_uint32,
                                    C.POINTER(EpisodesRequestC), C.POINTER(C.POINTER(EpisodesResultC))]),
    "mdb_episodes_result_free": (None, [C.POINTER(EpisodesResultC)]),
    "mdb_binned_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(SegmentsC), C.c_void_p,
                                     C.POINTER(BucketRequestC), C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_binned_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(SegmentsC), C.c_void_p,
                                         C.POINTER(BucketRequestC), C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_binned_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.c_uint32,
                                          C.POINTER(C.POINTER(SegmentsC)), C.c_uint32, C.POINTER(C.c_void_p),
                                          C.POINTER(BucketRequestC), C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_grid_count_filter_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(ValueFilterC),
                                            C.POINTER(C.c_uint64)]),
    "mdb_grid_batch_filter_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(ValueFilterC), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                            C.POINTER(GridMetricsC)]),
    "mdb_grid_batch_filter_owned": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(ValueFilterC), C.c_uint64,
                                              C.POINTER(C.POINTER(GridResultC))]),
    "mdb_agg_batch_filter": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(ValueFilterC), C.c_uint32,
                                       C.POINTER(AggStateC)]),
    "mdb_agg_batch_filter_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(ValueFilterC), C.c_uint32,
                                           C.POINTER(AggStateC)]),
    "mdb_agg_batch_filter_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.c_uint32,
                                            C.POINTER(ValueFilterC), C.c_uint32, C.POINTER(AggStateC)]),
    "mdb_agg_buckets_filter": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                         C.POINTER(ValueFilterC), C.c_void_p]),
    "mdb_agg_buckets_filter_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p,
                                             C.POINTER(BucketRequestC), C.POINTER(ValueFilterC), C.c_void_p]),
    "mdb_agg_buckets_filter_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p),
                                              C.c_uint32, C.POINTER(BucketRequestC), C.POINTER(ValueFilterC),
                                              C.c_void_p]),
    "mdb_mask_filter_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.POINTER(ValueFilterC), C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mdb_mask_combine_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.POINTER(C.c_uint64)]),
    "mdb_grid_batch_mask_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64, C.c_void_p, C.c_uint64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                          C.POINTER(GridMetricsC)]),
    "mdb_agg_batch_mask_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64, C.c_void_p, C.c_uint64,
                                         C.c_uint32, C.POINTER(AggStateC)]),
    "mdb_agg_batch_where": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(ValueFilterC), C.c_uint32,
                                      C.POINTER(SegmentsC), C.c_uint32, C.POINTER(AggStateC)]),
    "mdb_grid_batch_where_owned": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(ValueFilterC),
                                             C.c_uint32, C.POINTER(SegmentsC), C.c_uint32, C.c_uint64,
                                             C.POINTER(C.POINTER(GridResultC))]),
    "mdb_hist_batch": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(HistRequestC), C.c_void_p,
                                 C.c_void_p]),
    "mdb_hist_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(HistRequestC), C.c_void_p,
                                     C.c_void_p]),
    "mdb_hist_batch_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p), C.c_uint32,
                                      C.POINTER(HistRequestC), C.c_void_p, C.c_void_p]),
    "mdb_quantile_batch": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64, C.c_void_p, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "mdb_quantile_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_int64, C.c_int64, C.c_void_p, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "mdb_hist_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC), C.c_void_p,
                                   C.c_uint32, C.c_void_p]),
    "mdb_hist_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                       C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_hist_buckets_list": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(SegmentsC)), C.POINTER(C.c_void_p), C.c_uint32,
                                        C.POINTER(BucketRequestC), C.c_void_p, C.c_uint32, C.c_void_p]),
    "mdb_quantile_buckets": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                       C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mdb_quantile_buckets_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC), C.c_void_p, C.POINTER(BucketRequestC),
                                           C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mdb_hist_cell_of": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.POINTER(C.c_uint32)]),
    "mdb_quantile_positions": (C.c_int, [C.c_double, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_double)]),
    "mdb_compress_series": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, ErrorBoundC,
                                      C.POINTER(C.POINTER(SegmentsOwnedC))]),
    "mdb_compress_chunks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                      ErrorBoundC, C.POINTER(C.POINTER(SegmentsOwnedC))]),
    "mdb_compress_chunk_list": (C.c_int, [C.c_void_p, C.POINTER(ChunkC), C.c_uint64, ErrorBoundC,
                                          C.POINTER(C.POINTER(SegmentsOwnedC))]),
    "mdb_compress_chunks_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint64, ErrorBoundC, C.c_int64, C.c_int64,
                                          C.c_void_p, C.POINTER(C.POINTER(SegmentsOwnedC))]),
    "mdb_segments_validate_dev": (C.c_int, [C.c_void_p, C.POINTER(SegmentsC)]),
    "mdb_split_and_compress_univariate": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                                    C.POINTER(ErrorBoundC), C.c_uint32, C.c_uint64,
                                                    C.POINTER(C.POINTER(SegmentsOwnedC))]),
    "mdb_is_value_within_error_bound": (C.c_int, [ErrorBoundC, C.c_float, C.c_float,
                                                  C.POINTER(C.c_int32)]),
    "mdb_are_compressed_timestamps_regular": (C.c_int, [C.c_void_p, C.c_uint64,
                                                        C.POINTER(C.c_int32)]),
    "mdb_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mdb_comm_init": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "mdb_comm_close": (C.c_int, [C.c_void_p]),
    "mdb_agg_all_reduce": (C.c_int, [C.c_void_p, C.POINTER(AggStateC), C.POINTER(C.c_int32)]),
    "mdb_agg_merge": (C.c_int, [C.POINTER(AggStateC), C.POINTER(AggStateC)]),
    "mdb_agg_merge_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mdb_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "mdb_profile_reset": (C.c_int, [C.c_void_p]),
    "mdb_profile_get": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_double)]),
    "mdb_profile_names": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64]),
    "mdb_synth_values_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                       C.c_uint64]),
    "mdb_set_option": (C.c_int, [C.c_char_p, C.c_char_p]),
    "mdb_reload_options": (C.c_int, []),
    "mdb_option": (C.c_char_p, [C.c_char_p]),
}

_hip_library = None

# The library reads its switches (the MDB_* environment variables) once per process. Tests change os.environ from one
# call to the next: with this set (tests/conftest.py) every call through the binding is preceded by
# mdb_reload_options(), so that a test's monkeypatch.setenv() is seen by the call behind it.
RELOAD_OPTIONS_BEFORE_EVERY_CALL = False


class _ReloadingLibrary:
    """The ctypes library with mdb_reload_options() in front of every call while RELOAD_OPTIONS_BEFORE_EVERY_CALL."""

    def __init__(self, library):
        self._library = library

    def __getattr__(self, name):
        function = getattr(self._library, name)
        if not RELOAD_OPTIONS_BEFORE_EVERY_CALL or name in ("mdb_reload_options", "mdb_set_option", "mdb_option", "mdb_last_error"):
            return function
        reload_options = self._library.mdb_reload_options

        def call(*args):
            reload_options()
            return function(*args)

        return call


def hip_symbol_names():
    """Every symbol include/mdb.h declares (checked against the built library by the tests)."""
    return sorted(_HIP_SYMBOLS)


def load_hip_library():
    """Load libmdb_hip.so and declare its prototypes. Raises if it is missing: no fallback."""
    global _hip_library
    if _hip_library is not None:
        return _hip_library
    if not os.path.exists(HIP_LIBRARY_PATH):
        raise RuntimeError(
            f"{HIP_LIBRARY_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    library = C.CDLL(HIP_LIBRARY_PATH, mode=C.RTLD_GLOBAL)
    for name, (restype, argtypes) in _HIP_SYMBOLS.items():
        if "MDB_HIP_LIBRARY" in os.environ and not hasattr(library, name):
            continue  # A/B timing against an older build that predates a newer entry point
        function = getattr(library, name)  # AttributeError if the library lacks a declared symbol
        function.restype = restype
        function.argtypes = argtypes
    _hip_library = _ReloadingLibrary(library) if hasattr(library, "mdb_reload_options") else library
    return _hip_library
