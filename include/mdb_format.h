/*
 * mdb_format.h - constants and memory layouts of ModelarDB compressed segments.
 *
 * Pure C header shared by the HIP product library (modelardb-rs_amd/csrc), the host operators and
 * the CPU oracle (oracle/). Nothing here is executable; it restates the *format* the reference
 * defines so both sides agree on it.
 *
 * Reference sources restated (paths relative to the reference repository root):
 *   crates/modelardb_compression/src/models/mod.rs:36-50     model type ids, value size
 *   crates/modelardb_compression/src/compression.rs:38       RESIDUAL_VALUES_MAX_LENGTH
 *   crates/modelardb_types/src/types.rs:37-50,299-335        Timestamp=i64 us, Value=f32, ErrorBound
 *   crates/modelardb_types/src/schemas.rs:31-72              segment schema, metadata size (29)
 *   crates/modelardb_server/src/storage/mod.rs:58            65 536 point ingest buffers
 */
#ifndef MDB_FORMAT_H
#define MDB_FORMAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Model type ids (models/mod.rs:36-44). */
#define MDB_PMC_MEAN_ID 0
#define MDB_SWING_ID 1
#define MDB_MACAQUE_V_ID 2
#define MDB_MODEL_TYPE_COUNT 3

/* sizeof(Value) in bytes / bits (models/mod.rs:46-50). */
#define MDB_VALUE_SIZE_IN_BYTES 4
#define MDB_VALUE_SIZE_IN_BITS 32

/* Fixed-width bytes of one segment row: Int8 + 2*Timestamp + 3*Float32, BinaryView columns count
 * as 0 (schemas.rs:57-64 via arrow's primitive_width()). It only enters the bytes-per-value accept
 * test: PMC 29/len, Swing 30/len, accepted iff <= 4.0 (compression.rs:238). */
#define MDB_COMPRESSED_METADATA_SIZE_IN_BYTES 29

/* At most 255 residual values ride inside a model segment (compression.rs:38). */
#define MDB_RESIDUAL_VALUES_MAX_LENGTH 255

/* Points per ingest buffer handed to the compressor by the server (storage/mod.rs:58). */
#define MDB_UNCOMPRESSED_DATA_BUFFER_CAPACITY 65536

/* ErrorBound (types.rs:299-335). */
#define MDB_EB_LOSSLESS 0
#define MDB_EB_ABSOLUTE 1
#define MDB_EB_RELATIVE 2

typedef struct mdb_error_bound {
    int32_t kind; /* MDB_EB_* */
    float value;  /* absolute bound, or relative bound in percent; ignored for lossless */
} mdb_error_bound;

/* One Arrow BinaryView "view" (16 bytes). length <= 12: the bytes are inline (zero padded);
 * otherwise 4 prefix bytes, the index of the variadic data buffer and the offset into it. */
typedef struct mdb_view16 {
    int32_t length;
    union {
        uint8_t inlined[12];
        struct {
            uint8_t prefix[4];
            int32_t buffer_index;
            int32_t offset;
        } ref;
    } u;
} mdb_view16;

/* One Arrow BinaryViewArray column: views + its variadic data buffers, borrowed from Arrow. */
typedef struct mdb_binview_col {
    const mdb_view16 *views;       /* n views */
    const uint8_t *const *buffers; /* n_buffers data buffer base pointers (may be NULL if 0) */
    const int64_t *buffer_sizes;   /* n_buffers sizes in bytes (needed to stage to the device) */
    int32_t n_buffers;
} mdb_binview_col;

/* Struct-of-arrays view of a RecordBatch with QUERY_COMPRESSED_SCHEMA (schemas.rs:40-52):
 * 0 model_type_id | 1 start_time | 2 end_time | 3 timestamps | 4 min_value | 5 max_value |
 * 6 values | 7 residuals | (8 error: never read). Pointers go straight into Arrow buffers. */
typedef struct mdb_segments {
    uint64_t n;
    const int8_t *model_type_id;
    const int64_t *start_time;
    const int64_t *end_time;
    mdb_binview_col timestamps;
    const float *min_value;
    const float *max_value;
    mdb_binview_col values;
    mdb_binview_col residuals;
} mdb_segments;

/* Counters of GridStreamMetrics (query/grid_exec.rs:441-518). */
typedef struct mdb_grid_metrics {
    uint64_t rows_created;
    uint64_t rows_created_by_model_type[MDB_MODEL_TYPE_COUNT];
    uint64_t segments_with_residuals;
    uint64_t segments_with_model_type[MDB_MODEL_TYPE_COUNT];
    uint64_t segments_regular;
    uint64_t segments_irregular;
} mdb_grid_metrics;

/* Partial state of the five Model*Accumulators (optimizer/model_simple_aggregates.rs:336-618).
 * A fresh state is {0.0, 0, FLT_MAX, -FLT_MAX} (f32::MAX / f32::MIN, :413, :456). */
typedef struct mdb_agg_state {
    double sum;
    int64_t count;
    float min;
    float max;
} mdb_agg_state;

#define MDB_AGG_COUNT 1u
#define MDB_AGG_MIN 2u
#define MDB_AGG_MAX 4u
#define MDB_AGG_SUM 8u
#define MDB_AGG_AVG 16u

/* Segments produced by the compressor, owned by the library that made them: the nine columns of
 * COMPRESSED_SCHEMA minus the constant field_column/tag columns, BinaryView columns with one data
 * buffer each. `seg` aliases the owned memory so it can be passed straight back to grid/agg. */
typedef struct mdb_segments_owned {
    mdb_segments seg;
    const float *error;          /* always NaN (types.rs:265, compression.rs:398) */
    const uint32_t *chunk_index; /* which input chunk each segment came from */
    int32_t on_device;           /* 0: host pointers, 1: device pointers */
    void *priv_;                 /* owner's bookkeeping */
} mdb_segments_owned;

/* Reconstructed data points owned by the library: page-locked host memory (so the copy from the
 * device runs at the full PCIe rate) that the caller wraps without copying (e.g. arrow-rs
 * Buffer::from_custom_allocation) and returns with mdb_grid_result_free(). */
typedef struct mdb_grid_result {
    int64_t *timestamps;        /* n */
    float *values;              /* n */
    uint32_t *rows_per_segment; /* n_segments */
    uint64_t n;
    uint64_t n_segments;
    uint64_t reserved_front;    /* writable rows BEFORE timestamps[0] / values[0] (for leftovers) */
    mdb_grid_metrics metrics;
    void *priv_;
} mdb_grid_result;

/* One input RecordBatch of a pipelined grid call (mdb_grid_submit): its segment columns and, when the
 * stream's table has tag columns, the views of the batch's tag arrays (Utf8View: the same 16-byte
 * views, one per segment row), which the library repeats once per reconstructed data point. */
typedef struct mdb_grid_input {
    mdb_segments segments;
    const mdb_view16 *const *tag_views; /* n_tag_columns arrays of segments.n views; NULL without tags */
    /* n_tag_columns numbers added to buffer_index of every view longer than 12 bytes: the output tag
     * column's data buffers are [the caller's own buffers..., this batch's buffers...], and this is
     * where this batch's buffers start in that list. NULL: 0. */
    const int32_t *tag_buffer_shift;
} mdb_grid_input;

/* What to do with the inputs of one mdb_grid_submit. */
typedef struct mdb_grid_request {
    uint32_t flags;          /* MDB_GRID_HAS_RANGE | MDB_GRID_VALUES_ONLY */
    uint32_t n_tag_columns;  /* tag arrays per input */
    int64_t t_lo, t_hi;      /* with MDB_GRID_HAS_RANGE */
    uint64_t reserve_front;  /* writable rows in front of every output column (the leftovers) */
} mdb_grid_request;

/* Buckets of date_bin(width, ts, origin) for mdb_agg_buckets*: bucket b holds the points with
 * origin + b*width <= ts <= origin + (b+1)*width - 1, b = floor((ts - origin) / width) (floor, also for ts < origin). */
typedef struct mdb_bucket_request {
    int64_t  origin;
    int64_t  width;       /* > 0, in the timestamps' unit (us) */
    uint64_t n_buckets;   /* points outside buckets 0 .. n_buckets-1 are not counted */
    int64_t  t_lo, t_hi;  /* inclusive time range ANDed with the buckets (INT64_MIN / INT64_MAX: none) */
    uint32_t n_groups;    /* >= 1 */
    uint32_t which_mask;  /* MDB_AGG_*, with the same meaning as in mdb_agg_batch */
} mdb_bucket_request;     /* 48 bytes */

/* A value predicate ANDed with a time range, for mdb_grid_*_filter* and mdb_agg_batch_filter*: a point (t, v) passes
 * if t_lo <= t <= t_hi and v lies within [v_lo, v_hi] (ends open or absent per flags). The value bounds are compared
 * in IEEE 754 totalOrder on the f32 bit pattern (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN): the key
 * bits ^ ((int32_t)bits >> 31 & 0x7fffffff), compared as signed integers - the order of arrow-rs's float
 * comparison kernels, which DataFusion's FilterExec uses. IEEE v > c (never NaN) is (c, +inf]. */
#define MDB_VALUE_LO_OPEN 1u   /* v >  v_lo instead of v >= v_lo */
#define MDB_VALUE_HI_OPEN 2u   /* v <  v_hi instead of v <= v_hi */
#define MDB_VALUE_NO_LO   4u   /* no lower bound */
#define MDB_VALUE_NO_HI   8u   /* no upper bound */
typedef struct mdb_value_filter {
    int64_t  t_lo, t_hi;   /* inclusive time range, ANDed (INT64_MIN / INT64_MAX: none) */
    float    v_lo, v_hi;   /* value bounds */
    uint32_t flags;        /* MDB_VALUE_* */
    uint32_t reserved;     /* must be 0 */
} mdb_value_filter;        /* 32 bytes */

/* A value histogram for mdb_hist_batch*: n_edges edges (floats in a host array, strictly increasing in the totalOrder of
 * mdb_value_filter) cut the values into n_edges + 1 cells; a point of value v falls in cell c = the number of edges e
 * with key(e) <= key(v): cell 0 holds the points below the first edge, cell n_edges the points at or above the last.
 * 4 095 edges give 4 096 cells: 16 KB of keys in LDS, and three passes of 12 + 12 + 8 bits cover the 32-bit keys. */
#define MDB_HIST_MAX_EDGES 4095u
typedef struct mdb_hist_request {
    int64_t  t_lo, t_hi;   /* inclusive time range (INT64_MIN / INT64_MAX: none) */
    uint32_t n_edges;      /* 1 .. MDB_HIST_MAX_EDGES */
    uint32_t n_groups;     /* >= 1 */
    uint32_t flags;        /* must be 0 */
    uint32_t reserved;     /* must be 0 */
} mdb_hist_request;        /* 32 bytes */

/* One cell of mdb_m4_buckets*: the first, last, lowest and highest point of a bucket and group, with their timestamps
 * (the M4 aggregation: a line chart of the cell's points is redrawn exactly from these four). A fresh cell is all-zero
 * bytes. count == 0: the cell is empty and no other member is read; all are written when its first point arrives. */
typedef struct mdb_m4_cell {
    int64_t count;
    int64_t t_first, t_last, t_min, t_max;
    float   v_first, v_last, v_min, v_max;
} mdb_m4_cell;             /* 56 bytes */

/* One cell of mdb_moments_buckets*: the count, the mean and m2 = the sum of (v - mean)^2 over the points of a bucket
 * and group - the state DataFusion's variance accumulators keep (count, mean, m2), from which var_pop, var_samp and
 * the two stddev follow (mdb_moments_variance). A fresh cell is all-zero bytes. count == 0: the cell is empty and no
 * other member is read; all are written when its first points arrive. */
typedef struct mdb_moments_cell {
    int64_t count;
    double  mean;
    double  m2;
} mdb_moments_cell;        /* 24 bytes */

/* One cell of mdb_comoments_buckets*: the pairs (x, y) of a bucket and group - two fields of one table, paired row by
 * row. (count, mean_x, m2_x) and (count, mean_y, m2_y) are the states of DataFusion's variance accumulators of either
 * field, c_xy with the two means the state of its covariance accumulator: covar_pop / covar_samp, corr and regr_*
 * follow (mdb_comoments_finish). A fresh cell is all-zero bytes. count == 0: the cell is empty and no other member is
 * read; all are written when its first pairs arrive. */
typedef struct mdb_comoments_cell {
    int64_t count;
    double  mean_x, mean_y;
    double  m2_x, m2_y;   /* sum (x - mean_x)^2, sum (y - mean_y)^2 */
    double  c_xy;         /* sum (x - mean_x) * (y - mean_y) */
} mdb_comoments_cell;      /* 48 bytes */

/* The expression of mdb_derived_*: a generated field z = f(x, y) of two fields (FIELD AS (column_one + column_two)).
 * Every operation is one IEEE-754 binary32 operation, rounded to nearest, in the written order; nothing is fused,
 * denormals are kept (operands and results) and the division is the correctly rounded one. Zeros follow from the
 * formula as written and are not special-cased: c = +0 turns a -0 sum into +0, c = -0 keeps it. a, b and c must be
 * finite; an unknown op or flag bit is an error. */
#define MDB_DERIVED_LINEAR  0u   /* z = ((a * x) + (b * y)) + c */
#define MDB_DERIVED_PRODUCT 1u   /* z = (a * (x * y)) + c        (b is not read) */
#define MDB_DERIVED_RATIO   2u   /* z = (a * (x / y)) + c        (b is not read) */
#define MDB_DERIVED_ABS     1u   /* flag: z = |z| (sign bit cleared, also of a NaN) */
typedef struct mdb_derived_expr {
    uint32_t op;          /* MDB_DERIVED_LINEAR / _PRODUCT / _RATIO */
    uint32_t flags;       /* 0 or MDB_DERIVED_ABS */
    float    a, b, c;
} mdb_derived_expr;        /* 20 bytes */

/* One cell of mdb_derived_buckets*: the count, the mean and m2 = the sum of (z - mean)^2 of the generated values z of
 * a bucket and group, and their extremes. A fresh cell is all-zero bytes. count == 0: the cell is empty and no other
 * member is read or meaningful; all are written when its first values arrive.
 * count, mean, m2: the rules of mdb_moments_cell. min, max: the rule of mdb_agg_buckets' MIN and MAX - a run starts
 * at min = FLT_MAX, max = -FLT_MAX and takes a value by min = (z < min) ? z : min, max = (z > max) ? z : max, so a
 * NaN is skipped (a cell of NaNs only keeps FLT_MAX / -FLT_MAX, and FLT_MAX stays the min of a cell of +inf only),
 * and -0.0 and +0.0 compare equal: the one met first stays. */
typedef struct mdb_derived_cell {
    int64_t count;
    double  mean;
    double  m2;
    float   min;
    float   max;
} mdb_derived_cell;        /* 32 bytes */

/* One cell of mdb_integral_buckets*: the series of a bucket and group taken as a function of time. duration: the
 * microseconds of the bucket on which the function is defined (the clipped linked intervals, mdb.h), exact; integral:
 * the integral of the function over them, in value * microseconds. The time-weighted average is integral / duration
 * (mdb_integral_average). A fresh cell is all-zero bytes; cells merge by adding both members. */
typedef struct mdb_integral_cell {
    uint64_t duration;
    double   integral;
} mdb_integral_cell;       /* 16 bytes */

#define MDB_INTEGRAL_LINEAR 0u   /* trapezoid: the value between two linked points is interpolated */
#define MDB_INTEGRAL_STEP   1u   /* last observation carried forward */

typedef struct mdb_integral_request {   /* 64 bytes */
    mdb_bucket_request buckets;  /* t_lo / t_hi must be INT64_MIN / INT64_MAX, which_mask 0: the buckets are the range */
    int64_t  max_gap;            /* >= 0; INT64_MAX: no gap rule */
    uint32_t method;             /* MDB_INTEGRAL_* */
    uint32_t flags;              /* must be 0 */
} mdb_integral_request;

/* One cell of mdb_sample_at*: the value of the series of a group at one instant. count: the contributions the instant
 * received (rows on it, linked intervals around it, mdb.h), exact; sum: their values added as f64. The sampled value
 * is sum / count (mdb_sample_values). A fresh cell is all-zero bytes; a cell that has received nothing takes the other
 * whole when two merge, else both members are added. */
typedef struct mdb_sample_cell {
    uint64_t count;
    double   sum;
} mdb_sample_cell;         /* 16 bytes */

#define MDB_SAMPLE_LINEAR 0u   /* interpolate between two linked rows */
#define MDB_SAMPLE_STEP   1u   /* last observation carried forward over a linked interval */
#define MDB_SAMPLE_EXACT  2u   /* only rows that lie on an instant; nothing between rows */

typedef struct mdb_sample_request {     /* 64 bytes, laid out like mdb_integral_request */
    mdb_bucket_request instants; /* instant k is origin + k*width, k < n_buckets; t_lo / t_hi INT64_MIN / INT64_MAX, which_mask 0 */
    int64_t  max_gap;            /* >= 0; INT64_MAX: no gap rule */
    uint32_t method;             /* MDB_SAMPLE_* */
    uint32_t flags;              /* must be 0 */
} mdb_sample_request;

/* One cell of mdb_change_buckets*: the linked pairs of consecutive rows (mdb.h) whose LATER row lies in the bucket,
 * with d = (double)v1 - (double)v0 per pair. count, n_fall and duration are exact; the three sums are f64 additions;
 * the two maxima are bit-exact. A fresh cell is all-zero bytes; cells merge by adding the integers and the sums and
 * taking the larger of each maximum (mdb_change_merge_n). */
typedef struct mdb_change_cell {
    uint64_t count;      /* the pairs */
    uint64_t n_fall;     /* of which d < 0: the restarts of a counter */
    uint64_t duration;   /* sum of ts(r+1) - ts(r), microseconds */
    double   rise;       /* sum of d where d > 0 */
    double   fall;       /* sum of -d where d < 0 */
    double   reset_sum;  /* sum of (double)v1 where d < 0: what a restarted counter has counted since */
    double   max_rise;   /* the largest d > 0, else 0 */
    double   max_fall;   /* the largest -d where d < 0, else 0 */
} mdb_change_cell;         /* 64 bytes */

#define MDB_CHANGE_NET       0u  /* rise - fall */
#define MDB_CHANGE_VARIATION 1u  /* rise + fall: the total variation */
#define MDB_CHANGE_INCREASE  2u  /* rise + reset_sum: the increase of a counter that may restart */
#define MDB_CHANGE_RATE      3u  /* the increase per second: (rise + reset_sum) * 1e6 / duration */

typedef struct mdb_change_request {     /* 64 bytes, laid out like mdb_integral_request */
    mdb_bucket_request buckets;  /* t_lo / t_hi must be INT64_MIN / INT64_MAX, which_mask 0: the buckets are the range */
    int64_t  max_gap;            /* >= 0; INT64_MAX: no gap rule */
    uint32_t reserved;           /* must be 0 */
    uint32_t flags;              /* must be 0 */
} mdb_change_request;

#define MDB_DWELL_STEP 1u   /* the earlier value of a linked interval is held up to the later row: MDB_INTEGRAL_STEP's number */

/* The request of mdb_dwell_buckets*: the time spent per value cell. Its output is uint64_t microseconds, no cell struct. */
typedef struct mdb_dwell_request {      /* 64 bytes, laid out like mdb_integral_request */
    mdb_bucket_request buckets;  /* t_lo / t_hi must be INT64_MIN / INT64_MAX, which_mask 0: the buckets are the range */
    int64_t  max_gap;            /* >= 0; INT64_MAX: no gap rule */
    uint32_t method;             /* MDB_DWELL_STEP */
    uint32_t flags;              /* must be 0 */
} mdb_dwell_request;

/* The request of mdb_transit_buckets*: transitions between value cells. Its output is uint64_t counters, no cell struct. */
typedef struct mdb_transit_request {    /* 64 bytes, laid out like mdb_change_request */
    mdb_bucket_request buckets;  /* t_lo / t_hi must be INT64_MIN / INT64_MAX, which_mask 0: the buckets are the range */
    int64_t  max_gap;            /* >= 0; INT64_MAX: no gap rule */
    uint32_t reserved;           /* must be 0 */
    uint32_t flags;              /* must be 0 */
} mdb_transit_request;

/* The request of mdb_roll_cells*: overlapping windows of `window` adjacent buckets every `stride` buckets over cells
 * that a per-bucket operator has made. The cells are viewed as row-major [n_outer][n_buckets][n_inner] - the bucket
 * axis is the middle one; n_inner is 1 for [group][bucket] cells, the number of value cells (or its square) for the
 * counters of mdb_hist_buckets, mdb_dwell_buckets and mdb_transit_buckets and for the cells of mdb_binned_buckets. The
 * kind names the cell type and with it the merge rule, which is the operator's own:
 *   MDB_ROLL_AGG        mdb_agg_state, 24 B       mdb_agg_buckets*                      (mdb_agg_merge_n)
 *   MDB_ROLL_M4         mdb_m4_cell, 56 B         mdb_m4_buckets*                       (mdb_m4_merge_n)
 *   MDB_ROLL_MOMENTS    mdb_moments_cell, 24 B    mdb_moments_buckets*, mdb_binned_buckets*   (mdb_moments_merge_n)
 *   MDB_ROLL_COMOMENTS  mdb_comoments_cell, 48 B  mdb_comoments_buckets*, mdb_trend_buckets*  (mdb_comoments_merge_n)
 *   MDB_ROLL_DERIVED    mdb_derived_cell, 32 B    mdb_derived_buckets*                  (mdb_derived_merge_n)
 *   MDB_ROLL_INTEGRAL   mdb_integral_cell, 16 B   mdb_integral_buckets*                 (mdb_integral_merge_n)
 *   MDB_ROLL_CHANGE     mdb_change_cell, 64 B     mdb_change_buckets*                   (mdb_change_merge_n)
 *   MDB_ROLL_U64        uint64_t, 8 B             mdb_hist_buckets*, mdb_dwell_buckets*, mdb_transit_buckets* (wrapping add)
 * mdb_sample_cell has no kind: its cells belong to instants, not to intervals, and a window of instants is not the
 * merge of its instants' cells in any sense a query asks for. */
#define MDB_ROLL_AGG       0u
#define MDB_ROLL_M4        1u
#define MDB_ROLL_MOMENTS   2u
#define MDB_ROLL_COMOMENTS 3u
#define MDB_ROLL_DERIVED   4u
#define MDB_ROLL_INTEGRAL  5u
#define MDB_ROLL_CHANGE    6u
#define MDB_ROLL_U64       7u
typedef struct mdb_roll_request {       /* 48 bytes */
    uint32_t kind;       /* MDB_ROLL_* */
    uint32_t flags;      /* must be 0 */
    uint64_t n_outer;
    uint64_t n_buckets;
    uint64_t n_inner;
    uint64_t window;     /* buckets per window, >= 1 */
    uint64_t stride;     /* buckets between the starts of two windows, >= 1 */
} mdb_roll_request;

/* One series chunk of mdb_compress_chunk_list: n sorted data points in two arrays of the caller. */
typedef struct mdb_chunk {
    const int64_t *ts;
    const float *values;
    uint64_t n;
} mdb_chunk;

#ifdef __cplusplus
}
#endif

/* The layouts above are the ABI: pinned here for C and C++ and, with the same numbers, as `const`
 * assertions in rust/modelardb_hip/src/sys.rs and in tests/test_abi_cpu.py (ctypes). */
#include <stddef.h>
#ifdef __cplusplus
#define MDB_LAYOUT_ASSERT(condition) static_assert(condition, #condition)
#else
#define MDB_LAYOUT_ASSERT(condition) _Static_assert(condition, #condition)
#endif
MDB_LAYOUT_ASSERT(sizeof(mdb_error_bound) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_error_bound, value) == 4);
MDB_LAYOUT_ASSERT(sizeof(mdb_view16) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_view16, u) == 4);
MDB_LAYOUT_ASSERT(sizeof(mdb_binview_col) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_binview_col, buffers) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_binview_col, buffer_sizes) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_binview_col, n_buffers) == 24);
MDB_LAYOUT_ASSERT(sizeof(mdb_segments) == 144);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments, model_type_id) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments, start_time) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments, end_time) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments, timestamps) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments, min_value) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments, max_value) == 72);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments, values) == 80);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments, residuals) == 112);
MDB_LAYOUT_ASSERT(sizeof(mdb_grid_metrics) == 80);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_metrics, rows_created_by_model_type) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_metrics, segments_with_residuals) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_metrics, segments_with_model_type) == 40);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_metrics, segments_regular) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_metrics, segments_irregular) == 72);
MDB_LAYOUT_ASSERT(sizeof(mdb_agg_state) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_agg_state, count) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_agg_state, min) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_agg_state, max) == 20);
MDB_LAYOUT_ASSERT(sizeof(mdb_segments_owned) == 176);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments_owned, error) == 144);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments_owned, chunk_index) == 152);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments_owned, on_device) == 160);
MDB_LAYOUT_ASSERT(offsetof(mdb_segments_owned, priv_) == 168);
MDB_LAYOUT_ASSERT(sizeof(mdb_grid_result) == 136);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_result, values) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_result, rows_per_segment) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_result, n) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_result, n_segments) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_result, reserved_front) == 40);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_result, metrics) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_result, priv_) == 128);
MDB_LAYOUT_ASSERT(sizeof(mdb_grid_input) == 160);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_input, tag_views) == 144);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_input, tag_buffer_shift) == 152);
MDB_LAYOUT_ASSERT(sizeof(mdb_grid_request) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_request, n_tag_columns) == 4);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_request, t_lo) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_request, t_hi) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_grid_request, reserve_front) == 24);
MDB_LAYOUT_ASSERT(sizeof(mdb_chunk) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_chunk, values) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_chunk, n) == 16);
MDB_LAYOUT_ASSERT(sizeof(mdb_bucket_request) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_bucket_request, width) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_bucket_request, n_buckets) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_bucket_request, t_lo) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_bucket_request, t_hi) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_bucket_request, n_groups) == 40);
MDB_LAYOUT_ASSERT(offsetof(mdb_bucket_request, which_mask) == 44);
MDB_LAYOUT_ASSERT(sizeof(mdb_value_filter) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_value_filter, t_hi) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_value_filter, v_lo) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_value_filter, v_hi) == 20);
MDB_LAYOUT_ASSERT(offsetof(mdb_value_filter, flags) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_value_filter, reserved) == 28);
MDB_LAYOUT_ASSERT(sizeof(mdb_hist_request) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_hist_request, t_hi) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_hist_request, n_edges) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_hist_request, n_groups) == 20);
MDB_LAYOUT_ASSERT(offsetof(mdb_hist_request, flags) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_hist_request, reserved) == 28);
MDB_LAYOUT_ASSERT(sizeof(mdb_m4_cell) == 56);
MDB_LAYOUT_ASSERT(offsetof(mdb_m4_cell, t_first) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_m4_cell, t_last) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_m4_cell, t_min) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_m4_cell, t_max) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_m4_cell, v_first) == 40);
MDB_LAYOUT_ASSERT(offsetof(mdb_m4_cell, v_last) == 44);
MDB_LAYOUT_ASSERT(offsetof(mdb_m4_cell, v_min) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_m4_cell, v_max) == 52);
MDB_LAYOUT_ASSERT(sizeof(mdb_moments_cell) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_moments_cell, mean) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_moments_cell, m2) == 16);
MDB_LAYOUT_ASSERT(sizeof(mdb_comoments_cell) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_comoments_cell, count) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_comoments_cell, mean_x) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_comoments_cell, mean_y) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_comoments_cell, m2_x) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_comoments_cell, m2_y) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_comoments_cell, c_xy) == 40);
MDB_LAYOUT_ASSERT(sizeof(mdb_derived_expr) == 20);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_expr, op) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_expr, flags) == 4);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_expr, a) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_expr, b) == 12);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_expr, c) == 16);
MDB_LAYOUT_ASSERT(sizeof(mdb_derived_cell) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_cell, count) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_cell, mean) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_cell, m2) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_cell, min) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_derived_cell, max) == 28);
MDB_LAYOUT_ASSERT(sizeof(mdb_integral_cell) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_integral_cell, integral) == 8);
MDB_LAYOUT_ASSERT(sizeof(mdb_integral_request) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_integral_request, max_gap) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_integral_request, method) == 56);
MDB_LAYOUT_ASSERT(offsetof(mdb_integral_request, flags) == 60);
MDB_LAYOUT_ASSERT(sizeof(mdb_sample_cell) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_sample_cell, count) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_sample_cell, sum) == 8);
MDB_LAYOUT_ASSERT(sizeof(mdb_sample_request) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_sample_request, instants) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_sample_request, max_gap) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_sample_request, method) == 56);
MDB_LAYOUT_ASSERT(offsetof(mdb_sample_request, flags) == 60);
MDB_LAYOUT_ASSERT(sizeof(mdb_change_cell) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_cell, count) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_cell, n_fall) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_cell, duration) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_cell, rise) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_cell, fall) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_cell, reset_sum) == 40);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_cell, max_rise) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_cell, max_fall) == 56);
MDB_LAYOUT_ASSERT(sizeof(mdb_change_request) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_request, buckets) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_request, max_gap) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_request, reserved) == 56);
MDB_LAYOUT_ASSERT(offsetof(mdb_change_request, flags) == 60);
MDB_LAYOUT_ASSERT(sizeof(mdb_dwell_request) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_dwell_request, buckets) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_dwell_request, max_gap) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_dwell_request, method) == 56);
MDB_LAYOUT_ASSERT(offsetof(mdb_dwell_request, flags) == 60);
MDB_LAYOUT_ASSERT(sizeof(mdb_transit_request) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_transit_request, buckets) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_transit_request, max_gap) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_transit_request, reserved) == 56);
MDB_LAYOUT_ASSERT(offsetof(mdb_transit_request, flags) == 60);
MDB_LAYOUT_ASSERT(sizeof(mdb_roll_request) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_roll_request, kind) == 0);
MDB_LAYOUT_ASSERT(offsetof(mdb_roll_request, flags) == 4);
MDB_LAYOUT_ASSERT(offsetof(mdb_roll_request, n_outer) == 8);
MDB_LAYOUT_ASSERT(offsetof(mdb_roll_request, n_buckets) == 16);
MDB_LAYOUT_ASSERT(offsetof(mdb_roll_request, n_inner) == 24);
MDB_LAYOUT_ASSERT(offsetof(mdb_roll_request, window) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_roll_request, stride) == 40);

#endif /* MDB_FORMAT_H */
