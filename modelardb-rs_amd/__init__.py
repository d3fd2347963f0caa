"""MI355X-native implementation of ModelarDB's model-compression / grid / segment-aggregate path.

The directory name carries the reference's repository name, so it is imported either through the
``modelardb_rs_amd`` alias module at the repository root or with
``importlib.import_module("modelardb-rs_amd")``.
"""

from . import _abi, api, host, segment_files, segments, sharding  # noqa: F401
from ._abi import (  # noqa: F401
    MDB_AGG_AVG, MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM, MDB_MACAQUE_V_ID,
    MDB_MASK_AND, MDB_MASK_ANDNOT, MDB_MASK_NOT, MDB_MASK_OR, MDB_MASK_XOR,
    MDB_PMC_MEAN_ID, MDB_SWING_ID, MDB_VALUE_HI_OPEN, MDB_VALUE_LO_OPEN, MDB_VALUE_NO_HI, MDB_VALUE_NO_LO,
    MDB_CHANGE_INCREASE, MDB_CHANGE_NET, MDB_CHANGE_RATE, MDB_CHANGE_VARIATION, MDB_DWELL_STEP, MDB_DERIVED_ABS, MDB_DERIVED_CHUNK_ROWS, MDB_DERIVED_LINEAR, MDB_DERIVED_PRODUCT, MDB_DERIVED_RATIO, MDB_DERIVED_SHORT_ROWS, MDB_HIST_MAX_EDGES, MDB_INTEGRAL_LINEAR, MDB_INTEGRAL_STEP, MDB_SAMPLE_EXACT, MDB_SAMPLE_LINEAR, MDB_SAMPLE_STEP, MDB_QUANTILE_BUCKETS_MAX_Q, MDB_QUANTILE_BUCKETS_PASSES, MDB_ROLL_AGG, MDB_ROLL_CHANGE, MDB_ROLL_COMOMENTS, MDB_ROLL_DERIVED, MDB_ROLL_INTEGRAL, MDB_ROLL_M4, MDB_ROLL_MOMENTS, MDB_ROLL_U64, MODEL_TYPE_NAMES, HistRequestC, ComomentsCellC, DerivedCellC, DerivedExprC, M4CellC, MomentsCellC, RollRequestC, ValueFilterC, load_hip_library,
)
from .segments import BinaryViewColumn, SegmentBatch, error_bound  # noqa: F401
from .api import (  # noqa: F401
    AGG_STATE_DTYPE, CHANGE_CELL_DTYPE, COMOMENTS_CELL_DTYPE, DERIVED_CELL_DTYPE, DERIVED_OPS, EPISODE_DTYPE, INTEGRAL_CELL_DTYPE, SAMPLE_CELL_DTYPE, COMOMENTS_KINDS, M4_CELL_DTYPE, MOMENTS_CELL_DTYPE, Context, DeviceSegments, HipError, agg_merge_n, are_compressed_timestamps_regular,
    change_finish, change_merge, dwell_merge, dwell_share, transit_crossings, transit_merge, fresh_change_cells, comm_unique_id, comoments_finish, comoments_merge, comoments_moments, derived_apply, derived_expr, derived_merge, derived_stats, fresh_derived_cells, fresh_agg_states, fresh_comoments_cells, fresh_integral_cells, fresh_sample_cells, fresh_m4_cells, fresh_moments_cells, hist_cell_of, integral_average, integral_merge, sample_merge, sample_values, m4_merge, mask_words, moments_merge, moments_variance, quantile_positions, roll_cells, roll_kind_of, roll_windows, ROLL_KINDS, unpack_mask, is_value_within_error_bound, value_filter, value_filter_bits,
)
