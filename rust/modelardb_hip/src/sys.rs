//! Raw declarations of the C ABI in `include/mdb_format.h` and `include/mdb.h`.
//!
//! The struct names are the C names on purpose (`mdb_segments`, not `MdbSegments`): the layout
//! assertions at the end of this file carry the same numbers as the `MDB_LAYOUT_ASSERT` lines of
//! `include/mdb_format.h`, and `tests/test_abi_cpu.py` checks that the two lists agree.

#![allow(non_camel_case_types)]

use std::mem::{offset_of, size_of};
use std::os::raw::{c_char, c_int, c_void};

/// Opaque context: one HIP stream + scratch memory. Calls on one context are serialised inside the
/// library; use one context per `GridStream` / accumulator / compression thread.
#[repr(C)]
pub struct mdb_ctx {
    _private: [u8; 0],
}

pub const MDB_PMC_MEAN_ID: i8 = 0;
pub const MDB_SWING_ID: i8 = 1;
pub const MDB_MACAQUE_V_ID: i8 = 2;
pub const MDB_MODEL_TYPE_COUNT: usize = 3;

pub const MDB_EB_LOSSLESS: i32 = 0;
pub const MDB_EB_ABSOLUTE: i32 = 1;
pub const MDB_EB_RELATIVE: i32 = 2;

pub const MDB_AGG_COUNT: u32 = 1;
pub const MDB_AGG_MIN: u32 = 2;
pub const MDB_AGG_MAX: u32 = 4;
pub const MDB_AGG_SUM: u32 = 8;
pub const MDB_AGG_AVG: u32 = 16;

pub const MDB_GRID_HAS_RANGE: u32 = 1;
pub const MDB_GRID_VALUES_ONLY: u32 = 2;

pub const MDB_COMM_ID_BYTES: usize = 128;

/// `ErrorBound` (crates/modelardb_types/src/types.rs:299-335).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_error_bound {
    pub kind: i32,
    pub value: f32,
}

/// One Arrow BinaryView view: `length`, then 12 inline bytes or {prefix, buffer_index, offset}.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct mdb_view16 {
    pub length: i32,
    pub u: [u8; 12],
}

/// One `BinaryViewArray`: `views()`, `data_buffers()` base pointers and lengths.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct mdb_binview_col {
    pub views: *const mdb_view16,
    pub buffers: *const *const u8,
    pub buffer_sizes: *const i64,
    pub n_buffers: i32,
}

/// Struct-of-arrays view of a RecordBatch with `QUERY_COMPRESSED_SCHEMA`
/// (crates/modelardb_types/src/schemas.rs:40-52); pointers go straight into Arrow buffers.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct mdb_segments {
    pub n: u64,
    pub model_type_id: *const i8,
    pub start_time: *const i64,
    pub end_time: *const i64,
    pub timestamps: mdb_binview_col,
    pub min_value: *const f32,
    pub max_value: *const f32,
    pub values: mdb_binview_col,
    pub residuals: mdb_binview_col,
}

/// The counters of `GridStreamMetrics` (query/grid_exec.rs:441-518), per batch.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct mdb_grid_metrics {
    pub rows_created: u64,
    pub rows_created_by_model_type: [u64; MDB_MODEL_TYPE_COUNT],
    pub segments_with_residuals: u64,
    pub segments_with_model_type: [u64; MDB_MODEL_TYPE_COUNT],
    pub segments_regular: u64,
    pub segments_irregular: u64,
}

/// Partial state of the five `Model*Accumulator`s (optimizer/model_simple_aggregates.rs:336-618).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_agg_state {
    pub sum: f64,
    pub count: i64,
    pub min: f32,
    pub max: f32,
}

impl mdb_agg_state {
    /// `min: f32::MAX`, `max: f32::MIN` as in model_simple_aggregates.rs:413, 456.
    pub const FRESH: Self = Self { sum: 0.0, count: 0, min: f32::MAX, max: f32::MIN };
}

#[repr(C)]
pub struct mdb_segments_owned {
    pub seg: mdb_segments,
    pub error: *const f32,
    pub chunk_index: *const u32,
    pub on_device: i32,
    pub priv_: *mut c_void,
}

#[repr(C)]
pub struct mdb_grid_result {
    pub timestamps: *mut i64,
    pub values: *mut f32,
    pub rows_per_segment: *mut u32,
    pub n: u64,
    pub n_segments: u64,
    pub reserved_front: u64,
    pub metrics: mdb_grid_metrics,
    pub priv_: *mut c_void,
}

/// One input `RecordBatch` of a pipelined grid call: its segment columns and the views of its tag arrays.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct mdb_grid_input {
    pub segments: mdb_segments,
    /// `n_tag_columns` arrays of `segments.n` views (`StringViewArray::views()`), or null without tags.
    pub tag_views: *const *const mdb_view16,
    /// Per tag column: added to `buffer_index` of every view longer than 12 bytes; null means 0.
    pub tag_buffer_shift: *const i32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mdb_grid_request {
    pub flags: u32,
    pub n_tag_columns: u32,
    pub t_lo: i64,
    pub t_hi: i64,
    pub reserve_front: u64,
}

/// An outstanding `mdb_grid_submit`.
#[repr(C)]
pub struct mdb_grid_ticket {
    _private: [u8; 0],
}

/// One series chunk of `mdb_compress_chunk_list`: `n` sorted data points in two arrays of the caller.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct mdb_chunk {
    pub ts: *const i64,
    pub values: *const f32,
    pub n: u64,
}

/// The buckets of `date_bin(width, ts, origin)` for `mdb_agg_buckets*`: bucket b holds the points with
/// origin + b*width <= ts <= origin + (b+1)*width - 1 (floor division, also for ts < origin).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct mdb_bucket_request {
    pub origin: i64,
    /// > 0, in the timestamps' unit (µs).
    pub width: i64,
    /// Points outside buckets 0 .. n_buckets-1 are not counted.
    pub n_buckets: u64,
    /// Inclusive time range ANDed with the buckets (`i64::MIN` / `i64::MAX`: none).
    pub t_lo: i64,
    pub t_hi: i64,
    /// >= 1.
    pub n_groups: u32,
    /// `MDB_AGG_*`, as in `mdb_agg_batch`.
    pub which_mask: u32,
}

/// Operations of `mdb_mask_combine_dev` on row masks (`out = a op b`; `MDB_MASK_NOT`: `~a`, `b` must be null).
pub const MDB_MASK_AND: u32 = 0;
pub const MDB_MASK_OR: u32 = 1;
pub const MDB_MASK_XOR: u32 = 2;
pub const MDB_MASK_ANDNOT: u32 = 3;
pub const MDB_MASK_NOT: u32 = 4;

/// `mdb_value_filter` flags: an open lower / upper end, or none at all.
pub const MDB_VALUE_LO_OPEN: u32 = 1;
pub const MDB_VALUE_HI_OPEN: u32 = 2;
pub const MDB_VALUE_NO_LO: u32 = 4;
pub const MDB_VALUE_NO_HI: u32 = 8;

/// A value predicate ANDed with a time range for `mdb_grid_*_filter*` / `mdb_agg_batch_filter*`: a point passes if
/// t_lo <= t <= t_hi and its value lies within [v_lo, v_hi] (ends per `flags`), compared in IEEE 754 totalOrder on the
/// f32 bit pattern (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN), the order of arrow-rs's float kernels.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_value_filter {
    /// Inclusive time range (`i64::MIN` / `i64::MAX`: none).
    pub t_lo: i64,
    pub t_hi: i64,
    pub v_lo: f32,
    pub v_hi: f32,
    /// `MDB_VALUE_*`.
    pub flags: u32,
    /// Must be 0.
    pub reserved: u32,
}

/// Most edges of one histogram: 4 096 cells, 16 KB of keys in LDS, three passes cover the 32-bit keys.
pub const MDB_HIST_MAX_EDGES: u32 = 4095;
/// Most quantiles of one `mdb_quantile_buckets*` call, and the passes over the batch such a call makes (8 + 8 + 8 + 8
/// bits of the 32-bit keys), whatever the number of cells and ranks.
pub const MDB_QUANTILE_BUCKETS_MAX_Q: u32 = 4;
pub const MDB_QUANTILE_BUCKETS_PASSES: u32 = 4;

/// A value histogram for `mdb_hist_batch*`: `n_edges` edges (strictly increasing in the totalOrder of
/// `mdb_value_filter`) cut the values into `n_edges + 1` cells; a point falls in the cell numbered by the edges at or
/// below it.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct mdb_hist_request {
    /// Inclusive time range (`i64::MIN` / `i64::MAX`: none).
    pub t_lo: i64,
    pub t_hi: i64,
    /// 1 ..= `MDB_HIST_MAX_EDGES`.
    pub n_edges: u32,
    /// >= 1.
    pub n_groups: u32,
    /// Must be 0.
    pub flags: u32,
    /// Must be 0.
    pub reserved: u32,
}

/// One cell of `mdb_m4_buckets*`: the first, last, lowest and highest point of a bucket and group with their
/// timestamps, and the count. A fresh cell is all-zero bytes (`Default`); `count == 0`: empty, no other member is read.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_m4_cell {
    pub count: i64,
    pub t_first: i64,
    pub t_last: i64,
    pub t_min: i64,
    pub t_max: i64,
    pub v_first: f32,
    pub v_last: f32,
    pub v_min: f32,
    pub v_max: f32,
}

/// One cell of `mdb_comoments_buckets*`: the pairs `(x, y)` of a bucket and group. `(count, mean_x, m2_x)` and
/// `(count, mean_y, m2_y)` are the states of DataFusion's variance accumulators of either field, `c_xy` (the sum of
/// `(x - mean_x) * (y - mean_y)`) with the two means the state of its covariance accumulator. A fresh cell is all-zero
/// bytes (`Default`); `count == 0`: empty, no other member is read.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_comoments_cell {
    pub count: i64,
    pub mean_x: f64,
    pub mean_y: f64,
    pub m2_x: f64,
    pub m2_y: f64,
    pub c_xy: f64,
}

/// The expression of `mdb_derived_*`: `z = f(x, y)`, a generated field of two fields. Every operation is one binary32
/// operation in the written order; nothing is fused, denormals are kept, the division is the correctly rounded one.
/// `a`, `b` and `c` must be finite.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_derived_expr {
    pub op: u32,
    pub flags: u32,
    pub a: f32,
    pub b: f32,
    pub c: f32,
}

/// One cell of `mdb_derived_buckets*`: the count, the mean, `m2` (the sum of `(z - mean)^2`) and the extremes of the
/// generated values of a bucket and group. `count`, `mean`, `m2`: the rules of `mdb_moments_cell`; `min`, `max`: those
/// of `mdb_agg_buckets`' MIN and MAX. A fresh cell is all-zero bytes (`Default`); `count == 0`: empty, no other member
/// is read.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_derived_cell {
    pub count: i64,
    pub mean: f64,
    pub m2: f64,
    pub min: f32,
    pub max: f32,
}

/// The request of `mdb_roll_cells*`: windows of `window` adjacent buckets every `stride` buckets over cells viewed as
/// row-major `[n_outer][n_buckets][n_inner]`; `kind` (`MDB_ROLL_*`) names the cell type and its merge rule. 48 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_roll_request {
    pub kind: u32,
    pub flags: u32,
    pub n_outer: u64,
    pub n_buckets: u64,
    pub n_inner: u64,
    pub window: u64,
    pub stride: u64,
}

/// One episode of `mdb_episodes*`: a maximal run of consecutive passing rows, each but the first continuing its
/// predecessor (same group, time not stepping back, at most `max_gap` later). 64 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_episode {
    /// Row number in the range grid of the batch under the filter's time range (the row numbering of the masks).
    pub first_row: u64,
    pub count: u64,
    pub t_first: i64,
    pub t_last: i64,
    /// f64 sum of the f32 values.
    pub sum: f64,
    /// fmin / fmax from `f32::MAX` / `-f32::MAX`; a NaN is skipped.
    pub min: f32,
    pub max: f32,
    pub group: u32,
    /// Segment row of the batch (of the list) that holds `first_row`.
    pub first_segment: u32,
    pub reserved: u64,
}

/// The request of `mdb_episodes*`. 64 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_episodes_request {
    pub filter: mdb_value_filter,
    /// >= 0; `i64::MAX`: no gap rule.
    pub max_gap: i64,
    /// >= 0.
    pub min_duration: i64,
    /// 0 and 1: every episode.
    pub min_count: u64,
    /// >= 1.
    pub n_groups: u32,
    /// Must be 0.
    pub flags: u32,
}

#[repr(C)]
pub struct mdb_episodes_result {
    /// Host memory, `n` episodes (null if `n == 0`).
    pub episodes: *mut mdb_episode,
    pub n: u64,
    pub n_rows: u64,
    pub n_passing: u64,
    pub priv_: *mut c_void,
}

const _: () = assert!(std::mem::size_of::<mdb_episode>() == 64);
const _: () = assert!(std::mem::size_of::<mdb_episodes_request>() == 64);

/// One cell of `mdb_integral_buckets*`: the microseconds of a bucket on which the series is defined (the clipped
/// linked intervals) and the integral of the series over them, in value x microseconds. A fresh cell is all-zero bytes
/// (`Default`); cells merge by adding both members.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_integral_cell {
    pub duration: u64,
    pub integral: f64,
}

/// Trapezoid: the value between two linked points is interpolated.
pub const MDB_INTEGRAL_LINEAR: u32 = 0;
/// Last observation carried forward.
pub const MDB_INTEGRAL_STEP: u32 = 1;

/// The request of `mdb_integral_buckets*`. 64 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_integral_request {
    /// `t_lo` / `t_hi` must be `i64::MIN` / `i64::MAX` and `which_mask` 0: the buckets are the range.
    pub buckets: mdb_bucket_request,
    /// >= 0; `i64::MAX`: no gap rule.
    pub max_gap: i64,
    /// `MDB_INTEGRAL_*`.
    pub method: u32,
    /// Must be 0.
    pub flags: u32,
}

const _: () = assert!(std::mem::size_of::<mdb_integral_cell>() == 16);
const _: () = assert!(std::mem::offset_of!(mdb_integral_cell, integral) == 8);
const _: () = assert!(std::mem::size_of::<mdb_integral_request>() == 64);
const _: () = assert!(std::mem::offset_of!(mdb_integral_request, max_gap) == 48);
const _: () = assert!(std::mem::offset_of!(mdb_integral_request, method) == 56);
const _: () = assert!(std::mem::offset_of!(mdb_integral_request, flags) == 60);

/// One cell of `mdb_sample_at*`: the contributions an instant received (rows on it, linked intervals around it) and
/// their values added as f64; the sampled value is `sum / count`. A fresh cell is all-zero bytes (`Default`); a cell
/// with `count == 0` takes the other whole when two merge, else both members are added.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_sample_cell {
    pub count: u64,
    pub sum: f64,
}

/// Interpolate between two linked rows.
pub const MDB_SAMPLE_LINEAR: u32 = 0;
/// Last observation carried forward over a linked interval.
pub const MDB_SAMPLE_STEP: u32 = 1;
/// Only rows that lie on an instant; nothing between rows.
pub const MDB_SAMPLE_EXACT: u32 = 2;

/// The request of `mdb_sample_at*`. 64 bytes, laid out like `mdb_integral_request`.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_sample_request {
    /// Instant k is `origin + k * width`, `k < n_buckets`; `t_lo` / `t_hi` must be `i64::MIN` / `i64::MAX` and
    /// `which_mask` 0.
    pub instants: mdb_bucket_request,
    /// >= 0; `i64::MAX`: no gap rule.
    pub max_gap: i64,
    /// `MDB_SAMPLE_*`.
    pub method: u32,
    /// Must be 0.
    pub flags: u32,
}

const _: () = assert!(std::mem::size_of::<mdb_sample_cell>() == 16);
const _: () = assert!(std::mem::offset_of!(mdb_sample_cell, count) == 0);
const _: () = assert!(std::mem::offset_of!(mdb_sample_cell, sum) == 8);
const _: () = assert!(std::mem::size_of::<mdb_sample_request>() == 64);
const _: () = assert!(std::mem::offset_of!(mdb_sample_request, instants) == 0);
const _: () = assert!(std::mem::offset_of!(mdb_sample_request, max_gap) == 48);
const _: () = assert!(std::mem::offset_of!(mdb_sample_request, method) == 56);
const _: () = assert!(std::mem::offset_of!(mdb_sample_request, flags) == 60);

/// One cell of `mdb_change_buckets*`: the linked pairs of consecutive rows whose LATER row lies in the bucket, with
/// `d = v1 as f64 - v0 as f64` per pair. `count`, `n_fall` and `duration` are exact, the three sums f64 additions, the
/// two maxima bit-exact. A fresh cell is all-zero bytes (`Default`); cells merge by adding the integers and the sums
/// and taking the larger of each maximum.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_change_cell {
    /// The pairs.
    pub count: u64,
    /// Of which `d < 0`: the restarts of a counter.
    pub n_fall: u64,
    /// Sum of `ts(r+1) - ts(r)`, microseconds.
    pub duration: u64,
    /// Sum of `d` where `d > 0`.
    pub rise: f64,
    /// Sum of `-d` where `d < 0`.
    pub fall: f64,
    /// Sum of `v1` where `d < 0`: what a restarted counter has counted since.
    pub reset_sum: f64,
    /// The largest `d > 0`, else 0.
    pub max_rise: f64,
    /// The largest `-d` where `d < 0`, else 0.
    pub max_fall: f64,
}

/// `rise - fall`.
pub const MDB_CHANGE_NET: u32 = 0;
/// `rise + fall`: the total variation.
pub const MDB_CHANGE_VARIATION: u32 = 1;
/// `rise + reset_sum`: the increase of a counter that may restart.
pub const MDB_CHANGE_INCREASE: u32 = 2;
/// The increase per second: `(rise + reset_sum) * 1e6 / duration`.
pub const MDB_CHANGE_RATE: u32 = 3;

/// The request of `mdb_change_buckets*`. 64 bytes, laid out like `mdb_integral_request`.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_change_request {
    /// `t_lo` / `t_hi` must be `i64::MIN` / `i64::MAX` and `which_mask` 0: the buckets are the range.
    pub buckets: mdb_bucket_request,
    /// >= 0; `i64::MAX`: no gap rule.
    pub max_gap: i64,
    /// Must be 0.
    pub reserved: u32,
    /// Must be 0.
    pub flags: u32,
}

const _: () = assert!(std::mem::size_of::<mdb_change_cell>() == 64);
const _: () = assert!(std::mem::offset_of!(mdb_change_cell, count) == 0);
const _: () = assert!(std::mem::offset_of!(mdb_change_cell, n_fall) == 8);
const _: () = assert!(std::mem::offset_of!(mdb_change_cell, duration) == 16);
const _: () = assert!(std::mem::offset_of!(mdb_change_cell, rise) == 24);
const _: () = assert!(std::mem::offset_of!(mdb_change_cell, fall) == 32);
const _: () = assert!(std::mem::offset_of!(mdb_change_cell, reset_sum) == 40);
const _: () = assert!(std::mem::offset_of!(mdb_change_cell, max_rise) == 48);
const _: () = assert!(std::mem::offset_of!(mdb_change_cell, max_fall) == 56);
const _: () = assert!(std::mem::size_of::<mdb_change_request>() == 64);
const _: () = assert!(std::mem::offset_of!(mdb_change_request, buckets) == 0);
const _: () = assert!(std::mem::offset_of!(mdb_change_request, max_gap) == 48);
const _: () = assert!(std::mem::offset_of!(mdb_change_request, reserved) == 56);
const _: () = assert!(std::mem::offset_of!(mdb_change_request, flags) == 60);

/// The only method of `mdb_dwell_buckets*`: the earlier value of a linked interval is held up to the later row
/// (`MDB_INTEGRAL_STEP`'s number; 0, linear interpolation, is refused).
pub const MDB_DWELL_STEP: u32 = 1;

/// The request of `mdb_dwell_buckets*`. 64 bytes, laid out like `mdb_integral_request`.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_dwell_request {
    /// `t_lo` / `t_hi` must be `i64::MIN` / `i64::MAX` and `which_mask` 0: the buckets are the range.
    pub buckets: mdb_bucket_request,
    /// >= 0; `i64::MAX`: no gap rule.
    pub max_gap: i64,
    /// `MDB_DWELL_STEP`.
    pub method: u32,
    /// Must be 0.
    pub flags: u32,
}

const _: () = assert!(std::mem::size_of::<mdb_dwell_request>() == 64);
const _: () = assert!(std::mem::offset_of!(mdb_dwell_request, buckets) == 0);
const _: () = assert!(std::mem::offset_of!(mdb_dwell_request, max_gap) == 48);
const _: () = assert!(std::mem::offset_of!(mdb_dwell_request, method) == 56);
const _: () = assert!(std::mem::offset_of!(mdb_dwell_request, flags) == 60);

/// The request of `mdb_transit_buckets*`. 64 bytes, laid out like `mdb_change_request`.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct mdb_transit_request {
    /// `t_lo` / `t_hi` must be `i64::MIN` / `i64::MAX` and `which_mask` 0: the buckets are the range.
    pub buckets: mdb_bucket_request,
    /// >= 0; `i64::MAX`: no gap rule.
    pub max_gap: i64,
    /// Must be 0.
    pub reserved: u32,
    /// Must be 0.
    pub flags: u32,
}

const _: () = assert!(std::mem::size_of::<mdb_transit_request>() == 64);
const _: () = assert!(std::mem::offset_of!(mdb_transit_request, buckets) == 0);
const _: () = assert!(std::mem::offset_of!(mdb_transit_request, max_gap) == 48);
const _: () = assert!(std::mem::offset_of!(mdb_transit_request, reserved) == 56);
const _: () = assert!(std::mem::offset_of!(mdb_transit_request, flags) == 60);

/// The statistics of `mdb_comoments_finish`; x is the independent variable: SQL's `regr_*(y, x)`.
pub const MDB_COMOMENTS_COVAR_POP: u32 = 0;
pub const MDB_COMOMENTS_COVAR_SAMP: u32 = 1;
pub const MDB_COMOMENTS_CORR: u32 = 2;
pub const MDB_COMOMENTS_REGR_SLOPE: u32 = 3;
pub const MDB_COMOMENTS_REGR_INTERCEPT: u32 = 4;
pub const MDB_COMOMENTS_REGR_R2: u32 = 5;

/// The operations and the flag of `mdb_derived_expr`.
pub const MDB_DERIVED_LINEAR: u32 = 0; // z = ((a * x) + (b * y)) + c
pub const MDB_DERIVED_PRODUCT: u32 = 1; // z = (a * (x * y)) + c
pub const MDB_DERIVED_RATIO: u32 = 2; // z = (a * (x / y)) + c
pub const MDB_DERIVED_ABS: u32 = 1; // flag: z = |z|
/// How `mdb_derived_buckets*` cuts the rows: an interval of at most SHORT rows is one lane's, a longer one is cut
/// into chunks of CHUNK rows, one wave each.
pub const MDB_DERIVED_SHORT_ROWS: u32 = 64;
pub const MDB_DERIVED_CHUNK_ROWS: u32 = 1024;

/// The kinds of `mdb_roll_request`: the cell type and with it the merge rule. (`mdb_sample_cell` has none: instants
/// are not intervals.)
pub const MDB_ROLL_AGG: u32 = 0; // mdb_agg_state, 24 B
pub const MDB_ROLL_M4: u32 = 1; // mdb_m4_cell, 56 B
pub const MDB_ROLL_MOMENTS: u32 = 2; // mdb_moments_cell, 24 B (also binned)
pub const MDB_ROLL_COMOMENTS: u32 = 3; // mdb_comoments_cell, 48 B (also trend)
pub const MDB_ROLL_DERIVED: u32 = 4; // mdb_derived_cell, 32 B
pub const MDB_ROLL_INTEGRAL: u32 = 5; // mdb_integral_cell, 16 B
pub const MDB_ROLL_CHANGE: u32 = 6; // mdb_change_cell, 64 B
pub const MDB_ROLL_U64: u32 = 7; // u64, wrapping add (hist_buckets, dwell, transit)

/// One cell of `mdb_moments_buckets*`: the count, the mean and `m2`, the sum of `(v - mean)^2`, of a bucket and group:
/// the state of DataFusion's variance accumulators. A fresh cell is all-zero bytes (`Default`); `count == 0`: empty,
/// no other member is read.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct mdb_moments_cell {
    pub count: i64,
    pub mean: f64,
    pub m2: f64,
}

#[link(name = "mdb_hip")]
unsafe extern "C" {
    // ---- lifetime ----------------------------------------------------------------------------
    pub fn mdb_init(device: c_int, ctx: *mut *mut mdb_ctx) -> c_int;
    pub fn mdb_close(ctx: *mut mdb_ctx) -> c_int;
    pub fn mdb_clone(ctx: *mut mdb_ctx, out: *mut *mut mdb_ctx) -> c_int;
    pub fn mdb_last_error() -> *const c_char;
    pub fn mdb_version() -> *const c_char;
    pub fn mdb_set_stream(ctx: *mut mdb_ctx, hip_stream: *mut c_void) -> c_int;
    pub fn mdb_trim(ctx: *mut mdb_ctx, released_bytes: *mut u64) -> c_int;
    pub fn mdb_set_scratch_limit(ctx: *mut mdb_ctx, bytes: u64) -> c_int;
    pub fn mdb_device_info(ctx: *mut mdb_ctx, name: *mut c_char, name_cap: u64, compute_units: *mut i32,
                           hbm_bytes: *mut u64) -> c_int;

    // ---- device memory ---------------------------------------------------------------------------
    pub fn mdb_dev_alloc(ctx: *mut mdb_ctx, bytes: u64, dev_ptr: *mut *mut c_void) -> c_int;
    pub fn mdb_dev_free(ctx: *mut mdb_ctx, dev_ptr: *mut c_void) -> c_int;
    pub fn mdb_dev_upload(ctx: *mut mdb_ctx, dev_dst: *mut c_void, host_src: *const c_void, bytes: u64) -> c_int;
    pub fn mdb_dev_download(ctx: *mut mdb_ctx, host_dst: *mut c_void, dev_src: *const c_void, bytes: u64) -> c_int;
    pub fn mdb_dev_sync(ctx: *mut mdb_ctx) -> c_int;
    pub fn mdb_segments_upload(ctx: *mut mdb_ctx, host: *const mdb_segments, dev: *mut *mut mdb_segments_owned) -> c_int;
    pub fn mdb_segments_download(ctx: *mut mdb_ctx, dev: *const mdb_segments_owned,
                                 host: *mut *mut mdb_segments_owned) -> c_int;
    pub fn mdb_segments_free(segments: *mut mdb_segments_owned);
    pub fn mdb_segments_validate_dev(ctx: *mut mdb_ctx, dev: *const mdb_segments) -> c_int;

    // ---- grid (replaces the per-row loop of grid_exec.rs:323-356) ----------------------------------
    pub fn mdb_grid_count(ctx: *mut mdb_ctx, input: *const mdb_segments, n_out: *mut u64) -> c_int;
    pub fn mdb_grid_batch(ctx: *mut mdb_ctx, input: *const mdb_segments, out_ts: *mut i64, out_val: *mut f32,
                          out_rows_per_segment: *mut u32, cap: u64, n_out: *mut u64,
                          metrics: *mut mdb_grid_metrics) -> c_int;
    pub fn mdb_grid_count_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, n_out: *mut u64) -> c_int;
    pub fn mdb_grid_batch_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, out_ts: *mut i64, out_val: *mut f32,
                              out_rows_per_segment: *mut u32, cap: u64, n_out: *mut u64,
                              metrics: *mut mdb_grid_metrics) -> c_int;
    pub fn mdb_grid_count_range(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64,
                                n_out: *mut u64) -> c_int;
    pub fn mdb_grid_batch_range(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64,
                                out_ts: *mut i64, out_val: *mut f32, out_rows_per_segment: *mut u32, cap: u64,
                                n_out: *mut u64, metrics: *mut mdb_grid_metrics) -> c_int;
    pub fn mdb_grid_count_range_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64,
                                    n_out: *mut u64) -> c_int;
    pub fn mdb_grid_batch_range_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64,
                                    out_ts: *mut i64, out_val: *mut f32, out_rows_per_segment: *mut u32,
                                    cap: u64, n_out: *mut u64, metrics: *mut mdb_grid_metrics) -> c_int;
    pub fn mdb_grid_batch_owned(ctx: *mut mdb_ctx, input: *const mdb_segments, flags: u32, t_lo: i64, t_hi: i64,
                                reserve_front: u64, out: *mut *mut mdb_grid_result) -> c_int;
    pub fn mdb_grid_result_free(result: *mut mdb_grid_result);
    // (pipelined: several input batches per launch, two launches in flight, tag views replicated by the library)
    pub fn mdb_grid_submit(ctx: *mut mdb_ctx, inputs: *const mdb_grid_input, n_inputs: u32,
                           request: *const mdb_grid_request, ticket: *mut *mut mdb_grid_ticket) -> c_int;
    pub fn mdb_grid_wait(ticket: *mut mdb_grid_ticket, out: *mut *mut mdb_grid_result) -> c_int;
    pub fn mdb_grid_cancel(ticket: *mut mdb_grid_ticket);
    pub fn mdb_grid_result_tag_views(result: *const mdb_grid_result, column: u32) -> *mut mdb_view16;
    pub fn mdb_replicate_views(views: *const mdb_view16, rows_per_segment: *const u32, n_segments: u64,
                               buffer_shift: i32, out: *mut mdb_view16, out_cap: u64) -> c_int;

    // ---- the library's switches (read from the environment once per process; include/mdb.h) ----
    pub fn mdb_set_option(name: *const c_char, value: *const c_char) -> c_int;
    pub fn mdb_reload_options() -> c_int;
    pub fn mdb_option(name: *const c_char) -> *const c_char;

    // ---- aggregates (replace Model*Accumulator::update_batch, model_simple_aggregates.rs:345-587) ----
    pub fn mdb_agg_batch(ctx: *mut mdb_ctx, input: *const mdb_segments, which_mask: u32,
                         inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_batch_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, which_mask: u32,
                             inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_batch_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments, n_inputs: u32,
                              which_mask: u32, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_batch_range(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64,
                               which_mask: u32, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_batch_range_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64,
                                   which_mask: u32, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                           request: *const mdb_bucket_request, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                               request: *const mdb_bucket_request, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                group_of_segment: *const *const u32, n_inputs: u32,
                                request: *const mdb_bucket_request, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_grid_count_filter_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, filter: *const mdb_value_filter,
                                     n_out: *mut u64) -> c_int;
    pub fn mdb_grid_batch_filter_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, filter: *const mdb_value_filter,
                                     out_ts: *mut i64, out_val: *mut f32, out_rows_per_segment: *mut u32, cap: u64,
                                     n_out: *mut u64, metrics: *mut mdb_grid_metrics) -> c_int;
    pub fn mdb_grid_batch_filter_owned(ctx: *mut mdb_ctx, input: *const mdb_segments, filter: *const mdb_value_filter,
                                       reserve_front: u64, out: *mut *mut mdb_grid_result) -> c_int;
    pub fn mdb_agg_batch_filter(ctx: *mut mdb_ctx, input: *const mdb_segments, filter: *const mdb_value_filter,
                                which_mask: u32, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_batch_filter_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, filter: *const mdb_value_filter,
                                    which_mask: u32, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_batch_filter_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments, n_inputs: u32,
                                     filter: *const mdb_value_filter, which_mask: u32,
                                     inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_batch_range_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments, n_inputs: u32,
                                    t_lo: i64, t_hi: i64, which_mask: u32, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_buckets_filter(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                  request: *const mdb_bucket_request, filter: *const mdb_value_filter,
                                  inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_buckets_filter_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                      request: *const mdb_bucket_request, filter: *const mdb_value_filter,
                                      inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_buckets_filter_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                       group_of_segment: *const *const u32, n_inputs: u32,
                                       request: *const mdb_bucket_request, filter: *const mdb_value_filter,
                                       inout: *mut mdb_agg_state) -> c_int;
    // ---- row masks: a predicate on one field column selects the rows of another (include/mdb.h) ----
    pub fn mdb_mask_filter_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, filter: *const mdb_value_filter,
                               mask: *mut u64, cap_words: u64, n_rows: *mut u64, n_set: *mut u64) -> c_int;
    pub fn mdb_mask_combine_dev(ctx: *mut mdb_ctx, op: u32, a: *const u64, b: *const u64, out: *mut u64, n_rows: u64,
                                n_set: *mut u64) -> c_int;
    pub fn mdb_grid_batch_mask_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64,
                                   mask: *const u64, n_rows: u64, out_ts: *mut i64, out_val: *mut f32,
                                   out_rows_per_segment: *mut u32, cap: u64, n_out: *mut u64,
                                   metrics: *mut mdb_grid_metrics) -> c_int;
    pub fn mdb_agg_batch_mask_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64,
                                  mask: *const u64, n_rows: u64, which_mask: u32, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_agg_batch_where(ctx: *mut mdb_ctx, pred_fields: *const *const mdb_segments,
                               filters: *const mdb_value_filter, n_preds: u32, target: *const mdb_segments,
                               which_mask: u32, inout: *mut mdb_agg_state) -> c_int;
    pub fn mdb_grid_batch_where_owned(ctx: *mut mdb_ctx, pred_fields: *const *const mdb_segments,
                                      filters: *const mdb_value_filter, n_preds: u32, target: *const mdb_segments,
                                      flags: u32, reserve_front: u64, out: *mut *mut mdb_grid_result) -> c_int;
    // ---- value histograms and exact quantiles on segments (include/mdb.h) ----
    pub fn mdb_hist_batch(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                          request: *const mdb_hist_request, edges: *const f32, counts: *mut u64) -> c_int;
    pub fn mdb_hist_batch_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                              request: *const mdb_hist_request, edges: *const f32, counts: *mut u64) -> c_int;
    pub fn mdb_hist_batch_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                               group_of_segment: *const *const u32, n_inputs: u32, request: *const mdb_hist_request,
                               edges: *const f32, counts: *mut u64) -> c_int;
    pub fn mdb_m4_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                          request: *const mdb_bucket_request, inout: *mut mdb_m4_cell) -> c_int;
    pub fn mdb_m4_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                              request: *const mdb_bucket_request, inout: *mut mdb_m4_cell) -> c_int;
    pub fn mdb_m4_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                               group_of_segment: *const *const u32, n_inputs: u32, request: *const mdb_bucket_request,
                               inout: *mut mdb_m4_cell) -> c_int;
    pub fn mdb_m4_merge_n(into: *mut mdb_m4_cell, from: *const mdb_m4_cell, n: u64) -> c_int;
    pub fn mdb_moments_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                               request: *const mdb_bucket_request, inout: *mut mdb_moments_cell) -> c_int;
    pub fn mdb_moments_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                   request: *const mdb_bucket_request, inout: *mut mdb_moments_cell) -> c_int;
    pub fn mdb_moments_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                    group_of_segment: *const *const u32, n_inputs: u32,
                                    request: *const mdb_bucket_request, inout: *mut mdb_moments_cell) -> c_int;
    pub fn mdb_moments_merge_n(into: *mut mdb_moments_cell, from: *const mdb_moments_cell, n: u64) -> c_int;
    pub fn mdb_moments_variance(cells: *const mdb_moments_cell, n: u64, ddof: u32, variance_out: *mut f64) -> c_int;
    pub fn mdb_comoments_buckets(ctx: *mut mdb_ctx, x: *const mdb_segments, y: *const mdb_segments,
                                 group_of_segment_x: *const u32, request: *const mdb_bucket_request,
                                 inout: *mut mdb_comoments_cell) -> c_int;
    pub fn mdb_comoments_buckets_dev(ctx: *mut mdb_ctx, x: *const mdb_segments, y: *const mdb_segments,
                                     group_of_segment_x: *const u32, request: *const mdb_bucket_request,
                                     inout: *mut mdb_comoments_cell) -> c_int;
    pub fn mdb_comoments_buckets_list(ctx: *mut mdb_ctx, xs: *const *const mdb_segments, n_x: u32,
                                      ys: *const *const mdb_segments, n_y: u32,
                                      group_of_segment_x: *const *const u32, request: *const mdb_bucket_request,
                                      inout: *mut mdb_comoments_cell) -> c_int;
    pub fn mdb_comoments_merge_n(into: *mut mdb_comoments_cell, from: *const mdb_comoments_cell, n: u64) -> c_int;
    pub fn mdb_comoments_moments(cells: *const mdb_comoments_cell, n: u64, which: u32, out: *mut mdb_moments_cell) -> c_int;
    pub fn mdb_comoments_finish(cells: *const mdb_comoments_cell, n: u64, kind: u32, out: *mut f64) -> c_int;
    // ---- derived fields of two fields: z = f(x, y) as a column and per bucket (include/mdb.h) ----
    pub fn mdb_derived_values_dev(ctx: *mut mdb_ctx, x: *const mdb_segments, y: *const mdb_segments,
                                  expr: *const mdb_derived_expr, t_lo: i64, t_hi: i64, timestamps: *mut i64,
                                  values: *mut f32, capacity: u64, rows_out: *mut u64) -> c_int;
    pub fn mdb_derived_values(ctx: *mut mdb_ctx, x: *const mdb_segments, y: *const mdb_segments,
                              expr: *const mdb_derived_expr, t_lo: i64, t_hi: i64, timestamps: *mut i64,
                              values: *mut f32, capacity: u64, rows_out: *mut u64) -> c_int;
    pub fn mdb_derived_buckets(ctx: *mut mdb_ctx, x: *const mdb_segments, y: *const mdb_segments,
                               group_of_segment_x: *const u32, request: *const mdb_bucket_request,
                               expr: *const mdb_derived_expr, inout: *mut mdb_derived_cell) -> c_int;
    pub fn mdb_derived_buckets_dev(ctx: *mut mdb_ctx, x: *const mdb_segments, y: *const mdb_segments,
                                   group_of_segment_x: *const u32, request: *const mdb_bucket_request,
                                   expr: *const mdb_derived_expr, inout: *mut mdb_derived_cell) -> c_int;
    pub fn mdb_derived_buckets_list(ctx: *mut mdb_ctx, xs: *const *const mdb_segments, n_x: u32,
                                    ys: *const *const mdb_segments, n_y: u32,
                                    group_of_segment_x: *const *const u32, request: *const mdb_bucket_request,
                                    expr: *const mdb_derived_expr, inout: *mut mdb_derived_cell) -> c_int;
    pub fn mdb_derived_apply(expr: *const mdb_derived_expr, x: *const f32, y: *const f32, n: u64, z: *mut f32) -> c_int;
    pub fn mdb_derived_merge_n(into: *mut mdb_derived_cell, from: *const mdb_derived_cell, n: u64) -> c_int;
    pub fn mdb_derived_stats(cells: *const mdb_derived_cell, n: u64, out: *mut mdb_moments_cell) -> c_int;
    // ---- rolling windows over per-bucket cells: moving aggregates (include/mdb.h) ----
    pub fn mdb_roll_windows(request: *const mdb_roll_request, n_windows: *mut u64) -> c_int;
    pub fn mdb_roll_cells(request: *const mdb_roll_request, cells: *const c_void, out: *mut c_void,
                          capacity_cells: u64) -> c_int;
    pub fn mdb_roll_cells_dev(ctx: *mut mdb_ctx, request: *const mdb_roll_request, cells: *const c_void,
                              out: *mut c_void, capacity_cells: u64) -> c_int;
    // ---- linear trend of a field over time: comoments cells with x = the time offset in the bucket (include/mdb.h) ----
    pub fn mdb_trend_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                             request: *const mdb_bucket_request, inout: *mut mdb_comoments_cell) -> c_int;
    pub fn mdb_trend_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                 request: *const mdb_bucket_request, inout: *mut mdb_comoments_cell) -> c_int;
    pub fn mdb_trend_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                  group_of_segment: *const *const u32, n_inputs: u32,
                                  request: *const mdb_bucket_request, inout: *mut mdb_comoments_cell) -> c_int;
    // ---- time-weighted averages and integrals per bucket: the series as a function of time (include/mdb.h) ----
    pub fn mdb_integral_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                request: *const mdb_integral_request, inout: *mut mdb_integral_cell) -> c_int;
    pub fn mdb_integral_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                    request: *const mdb_integral_request, inout: *mut mdb_integral_cell) -> c_int;
    pub fn mdb_integral_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                     group_of_segment: *const *const u32, n_inputs: u32,
                                     request: *const mdb_integral_request, inout: *mut mdb_integral_cell) -> c_int;
    pub fn mdb_integral_merge_n(into: *mut mdb_integral_cell, from: *const mdb_integral_cell, n: u64) -> c_int;
    pub fn mdb_integral_average(cells: *const mdb_integral_cell, n: u64, out: *mut f64) -> c_int;

    // ---- the value of a series at regular instants: gap-fill, LOCF, interpolation (include/mdb.h) ----
    pub fn mdb_sample_at(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                         request: *const mdb_sample_request, inout: *mut mdb_sample_cell) -> c_int;
    pub fn mdb_sample_at_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                             request: *const mdb_sample_request, inout: *mut mdb_sample_cell) -> c_int;
    pub fn mdb_sample_at_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                              group_of_segment: *const *const u32, n_inputs: u32,
                              request: *const mdb_sample_request, inout: *mut mdb_sample_cell) -> c_int;
    pub fn mdb_sample_merge_n(into: *mut mdb_sample_cell, from: *const mdb_sample_cell, n: u64) -> c_int;
    pub fn mdb_sample_values(cells: *const mdb_sample_cell, n: u64, out: *mut f64) -> c_int;

    // ---- changes between consecutive points per bucket: increase, restarts, ramps, variation (include/mdb.h) ----
    pub fn mdb_change_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                              request: *const mdb_change_request, inout: *mut mdb_change_cell) -> c_int;
    pub fn mdb_change_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                  request: *const mdb_change_request, inout: *mut mdb_change_cell) -> c_int;
    pub fn mdb_change_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                   group_of_segment: *const *const u32, n_inputs: u32,
                                   request: *const mdb_change_request, inout: *mut mdb_change_cell) -> c_int;
    pub fn mdb_change_merge_n(into: *mut mdb_change_cell, from: *const mdb_change_cell, n: u64) -> c_int;
    pub fn mdb_change_finish(cells: *const mdb_change_cell, n: u64, kind: u32, out: *mut f64) -> c_int;

    // ---- the time spent per value cell, per bucket: time in state, load-duration curves (include/mdb.h) ----
    pub fn mdb_dwell_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                             request: *const mdb_dwell_request, edges: *const f32, n_edges: u32,
                             dwell: *mut u64) -> c_int;
    pub fn mdb_dwell_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                 request: *const mdb_dwell_request, edges: *const f32, n_edges: u32,
                                 dwell: *mut u64) -> c_int;
    pub fn mdb_dwell_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                  group_of_segment: *const *const u32, n_inputs: u32,
                                  request: *const mdb_dwell_request, edges: *const f32, n_edges: u32,
                                  dwell: *mut u64) -> c_int;
    pub fn mdb_dwell_merge_n(into: *mut u64, from: *const u64, n: u64) -> c_int;
    pub fn mdb_dwell_share(dwell: *const u64, n_rows: u64, n_cells: u32, out: *mut f64) -> c_int;

    // ---- transitions between value cells, per bucket: starts per day, level crossings (include/mdb.h) ----
    pub fn mdb_transit_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                               request: *const mdb_transit_request, edges: *const f32, n_edges: u32,
                               counts: *mut u64) -> c_int;
    pub fn mdb_transit_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                   request: *const mdb_transit_request, edges: *const f32, n_edges: u32,
                                   counts: *mut u64) -> c_int;
    pub fn mdb_transit_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                    group_of_segment: *const *const u32, n_inputs: u32,
                                    request: *const mdb_transit_request, edges: *const f32, n_edges: u32,
                                    counts: *mut u64) -> c_int;
    pub fn mdb_transit_merge_n(into: *mut u64, from: *const u64, n: u64) -> c_int;
    pub fn mdb_transit_crossings(counts: *const u64, n_rows: u64, n_cells: u32, up: *mut u64, down: *mut u64) -> c_int;
    // ---- episodes: the maximal runs of points that pass a value predicate (include/mdb.h) ----
    pub fn mdb_episodes_count_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                  request: *const mdb_episodes_request, n_episodes: *mut u64, n_rows: *mut u64,
                                  n_passing: *mut u64) -> c_int;
    pub fn mdb_episodes_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                            request: *const mdb_episodes_request, out: *mut mdb_episode, cap: u64, n_out: *mut u64,
                            n_rows: *mut u64, n_passing: *mut u64) -> c_int;
    pub fn mdb_episodes(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                        request: *const mdb_episodes_request, out: *mut *mut mdb_episodes_result) -> c_int;
    pub fn mdb_episodes_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                             group_of_segment: *const *const u32, n_inputs: u32,
                             request: *const mdb_episodes_request, out: *mut *mut mdb_episodes_result) -> c_int;
    pub fn mdb_episodes_result_free(result: *mut mdb_episodes_result);
    // ---- moments of one field per value cell of another (include/mdb.h) ----
    pub fn mdb_binned_buckets(ctx: *mut mdb_ctx, x: *const mdb_segments, y: *const mdb_segments,
                              group_of_segment_x: *const u32, request: *const mdb_bucket_request, edges: *const f32,
                              n_edges: u32, inout: *mut mdb_moments_cell) -> c_int;
    pub fn mdb_binned_buckets_dev(ctx: *mut mdb_ctx, x: *const mdb_segments, y: *const mdb_segments,
                                  group_of_segment_x: *const u32, request: *const mdb_bucket_request, edges: *const f32,
                                  n_edges: u32, inout: *mut mdb_moments_cell) -> c_int;
    pub fn mdb_binned_buckets_list(ctx: *mut mdb_ctx, xs: *const *const mdb_segments, n_x: u32,
                                   ys: *const *const mdb_segments, n_y: u32,
                                   group_of_segment_x: *const *const u32, request: *const mdb_bucket_request,
                                   edges: *const f32, n_edges: u32, inout: *mut mdb_moments_cell) -> c_int;
    pub fn mdb_quantile_batch(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64, q: *const f64,
                              n_q: u32, out_lo: *mut f32, out_hi: *mut f32, n_points: *mut u64) -> c_int;
    pub fn mdb_quantile_batch_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, t_lo: i64, t_hi: i64, q: *const f64,
                                  n_q: u32, out_lo: *mut f32, out_hi: *mut f32, n_points: *mut u64) -> c_int;
    // ---- histograms and exact quantiles per date_bin bucket and group (include/mdb.h) ----
    pub fn mdb_hist_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                            request: *const mdb_bucket_request, edges: *const f32, n_edges: u32, counts: *mut u64)
                            -> c_int;
    pub fn mdb_hist_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                request: *const mdb_bucket_request, edges: *const f32, n_edges: u32, counts: *mut u64)
                                -> c_int;
    pub fn mdb_hist_buckets_list(ctx: *mut mdb_ctx, inputs: *const *const mdb_segments,
                                 group_of_segment: *const *const u32, n_inputs: u32, request: *const mdb_bucket_request,
                                 edges: *const f32, n_edges: u32, counts: *mut u64) -> c_int;
    pub fn mdb_quantile_buckets(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                request: *const mdb_bucket_request, q: *const f64, n_q: u32, out_lo: *mut f32,
                                out_hi: *mut f32, n_points: *mut u64) -> c_int;
    pub fn mdb_quantile_buckets_dev(ctx: *mut mdb_ctx, input: *const mdb_segments, group_of_segment: *const u32,
                                    request: *const mdb_bucket_request, q: *const f64, n_q: u32, out_lo: *mut f32,
                                    out_hi: *mut f32, n_points: *mut u64) -> c_int;
    pub fn mdb_hist_cell_of(edges: *const f32, n_edges: u32, value: f32, cell: *mut u32) -> c_int;
    pub fn mdb_quantile_positions(q: f64, n_points: u64, rank_lo: *mut u64, rank_hi: *mut u64,
                                  fraction: *mut f64) -> c_int;

    // ---- fit (replaces try_compress_univariate_time_series, compression.rs:191-275) -----------------
    pub fn mdb_compress_series(ctx: *mut mdb_ctx, ts: *const i64, values: *const f32, n: u64,
                               error_bound: mdb_error_bound, out: *mut *mut mdb_segments_owned) -> c_int;
    pub fn mdb_compress_chunks(ctx: *mut mdb_ctx, ts: *const i64, values: *const f32, chunk_offsets: *const u64,
                               n_chunks: u64, error_bound: mdb_error_bound,
                               out: *mut *mut mdb_segments_owned) -> c_int;
    pub fn mdb_compress_chunk_list(ctx: *mut mdb_ctx, chunks: *const mdb_chunk, n_chunks: u64,
                                   error_bound: mdb_error_bound, out: *mut *mut mdb_segments_owned) -> c_int;
    pub fn mdb_compress_chunks_dev(ctx: *mut mdb_ctx, ts: *const i64, values: *const f32,
                                   chunk_offsets: *const u64, n_chunks: u64, error_bound: mdb_error_bound,
                                   regular_start: i64, regular_interval: i64, series_first_index: *const u64,
                                   out: *mut *mut mdb_segments_owned) -> c_int;
    pub fn mdb_split_and_compress_univariate(ctx: *mut mdb_ctx, ts: *const i64, field_values: *const *const f32,
                                             error_bounds: *const mdb_error_bound, n_fields: u32, n: u64,
                                             out: *mut *mut mdb_segments_owned) -> c_int;

    // ---- the crate's remaining public helpers (lib.rs:30-33), host arithmetic ------------------------
    pub fn mdb_is_value_within_error_bound(error_bound: mdb_error_bound, real_value: f32, approximate_value: f32,
                                           within: *mut i32) -> c_int;
    pub fn mdb_are_compressed_timestamps_regular(compressed_timestamps: *const u8, n_bytes: u64,
                                                 regular: *mut i32) -> c_int;

    // ---- multi-GPU: the final aggregate merge over RCCL / xGMI ---------------------------------------
    pub fn mdb_comm_unique_id(id_out: *mut c_void) -> c_int;
    pub fn mdb_comm_init(ctx: *mut mdb_ctx, rank: i32, world: i32, unique_id: *const c_void) -> c_int;
    pub fn mdb_comm_close(ctx: *mut mdb_ctx) -> c_int;
    pub fn mdb_agg_all_reduce(ctx: *mut mdb_ctx, inout: *mut mdb_agg_state, ranks_seen: *mut i32) -> c_int;
    pub fn mdb_agg_merge(into: *mut mdb_agg_state, from: *const mdb_agg_state) -> c_int;
    pub fn mdb_agg_merge_n(into: *mut mdb_agg_state, from: *const mdb_agg_state, n: u64) -> c_int;

    // ---- measurement ---------------------------------------------------------------------------------
    pub fn mdb_profile_enable(ctx: *mut mdb_ctx, enabled: c_int) -> c_int;
    pub fn mdb_profile_reset(ctx: *mut mdb_ctx) -> c_int;
    pub fn mdb_profile_get(ctx: *mut mdb_ctx, name: *const c_char, launches: *mut u64, total_ms: *mut f64) -> c_int;
    pub fn mdb_profile_names(ctx: *mut mdb_ctx, out: *mut c_char, cap: u64) -> c_int;
    pub fn mdb_synth_values_dev(ctx: *mut mdb_ctx, out: *mut f32, first_series: u64, n_series: u64,
                                n_per_series: u64, seed: u64) -> c_int;
}

// ---- layouts: the same numbers as the MDB_LAYOUT_ASSERT lines of include/mdb_format.h -----------------
const _: () = assert!(size_of::<mdb_error_bound>() == 8);
const _: () = assert!(offset_of!(mdb_error_bound, value) == 4);
const _: () = assert!(size_of::<mdb_view16>() == 16);
const _: () = assert!(offset_of!(mdb_view16, u) == 4);
const _: () = assert!(size_of::<mdb_binview_col>() == 32);
const _: () = assert!(offset_of!(mdb_binview_col, buffers) == 8);
const _: () = assert!(offset_of!(mdb_binview_col, buffer_sizes) == 16);
const _: () = assert!(offset_of!(mdb_binview_col, n_buffers) == 24);
const _: () = assert!(size_of::<mdb_segments>() == 144);
const _: () = assert!(offset_of!(mdb_segments, model_type_id) == 8);
const _: () = assert!(offset_of!(mdb_segments, start_time) == 16);
const _: () = assert!(offset_of!(mdb_segments, end_time) == 24);
const _: () = assert!(offset_of!(mdb_segments, timestamps) == 32);
const _: () = assert!(offset_of!(mdb_segments, min_value) == 64);
const _: () = assert!(offset_of!(mdb_segments, max_value) == 72);
const _: () = assert!(offset_of!(mdb_segments, values) == 80);
const _: () = assert!(offset_of!(mdb_segments, residuals) == 112);
const _: () = assert!(size_of::<mdb_grid_metrics>() == 80);
const _: () = assert!(offset_of!(mdb_grid_metrics, rows_created_by_model_type) == 8);
const _: () = assert!(offset_of!(mdb_grid_metrics, segments_with_residuals) == 32);
const _: () = assert!(offset_of!(mdb_grid_metrics, segments_with_model_type) == 40);
const _: () = assert!(offset_of!(mdb_grid_metrics, segments_regular) == 64);
const _: () = assert!(offset_of!(mdb_grid_metrics, segments_irregular) == 72);
const _: () = assert!(size_of::<mdb_agg_state>() == 24);
const _: () = assert!(offset_of!(mdb_agg_state, count) == 8);
const _: () = assert!(offset_of!(mdb_agg_state, min) == 16);
const _: () = assert!(offset_of!(mdb_agg_state, max) == 20);
const _: () = assert!(size_of::<mdb_segments_owned>() == 176);
const _: () = assert!(offset_of!(mdb_segments_owned, error) == 144);
const _: () = assert!(offset_of!(mdb_segments_owned, chunk_index) == 152);
const _: () = assert!(offset_of!(mdb_segments_owned, on_device) == 160);
const _: () = assert!(offset_of!(mdb_segments_owned, priv_) == 168);
const _: () = assert!(size_of::<mdb_grid_result>() == 136);
const _: () = assert!(offset_of!(mdb_grid_result, values) == 8);
const _: () = assert!(offset_of!(mdb_grid_result, rows_per_segment) == 16);
const _: () = assert!(offset_of!(mdb_grid_result, n) == 24);
const _: () = assert!(offset_of!(mdb_grid_result, n_segments) == 32);
const _: () = assert!(offset_of!(mdb_grid_result, reserved_front) == 40);
const _: () = assert!(offset_of!(mdb_grid_result, metrics) == 48);
const _: () = assert!(offset_of!(mdb_grid_result, priv_) == 128);
const _: () = assert!(size_of::<mdb_grid_input>() == 160);
const _: () = assert!(offset_of!(mdb_grid_input, tag_views) == 144);
const _: () = assert!(offset_of!(mdb_grid_input, tag_buffer_shift) == 152);
const _: () = assert!(size_of::<mdb_grid_request>() == 32);
const _: () = assert!(offset_of!(mdb_grid_request, n_tag_columns) == 4);
const _: () = assert!(offset_of!(mdb_grid_request, t_lo) == 8);
const _: () = assert!(offset_of!(mdb_grid_request, t_hi) == 16);
const _: () = assert!(offset_of!(mdb_grid_request, reserve_front) == 24);
const _: () = assert!(size_of::<mdb_chunk>() == 24);
const _: () = assert!(offset_of!(mdb_chunk, values) == 8);
const _: () = assert!(offset_of!(mdb_chunk, n) == 16);
const _: () = assert!(size_of::<mdb_bucket_request>() == 48);
const _: () = assert!(offset_of!(mdb_bucket_request, width) == 8);
const _: () = assert!(offset_of!(mdb_bucket_request, n_buckets) == 16);
const _: () = assert!(offset_of!(mdb_bucket_request, t_lo) == 24);
const _: () = assert!(offset_of!(mdb_bucket_request, t_hi) == 32);
const _: () = assert!(offset_of!(mdb_bucket_request, n_groups) == 40);
const _: () = assert!(offset_of!(mdb_bucket_request, which_mask) == 44);
const _: () = assert!(size_of::<mdb_value_filter>() == 32);
const _: () = assert!(offset_of!(mdb_value_filter, t_hi) == 8);
const _: () = assert!(offset_of!(mdb_value_filter, v_lo) == 16);
const _: () = assert!(offset_of!(mdb_value_filter, v_hi) == 20);
const _: () = assert!(offset_of!(mdb_value_filter, flags) == 24);
const _: () = assert!(offset_of!(mdb_value_filter, reserved) == 28);
const _: () = assert!(size_of::<mdb_hist_request>() == 32);
const _: () = assert!(offset_of!(mdb_hist_request, t_hi) == 8);
const _: () = assert!(offset_of!(mdb_hist_request, n_edges) == 16);
const _: () = assert!(offset_of!(mdb_hist_request, n_groups) == 20);
const _: () = assert!(offset_of!(mdb_hist_request, flags) == 24);
const _: () = assert!(offset_of!(mdb_hist_request, reserved) == 28);
const _: () = assert!(size_of::<mdb_m4_cell>() == 56);
const _: () = assert!(offset_of!(mdb_m4_cell, t_first) == 8);
const _: () = assert!(offset_of!(mdb_m4_cell, t_last) == 16);
const _: () = assert!(offset_of!(mdb_m4_cell, t_min) == 24);
const _: () = assert!(offset_of!(mdb_m4_cell, t_max) == 32);
const _: () = assert!(offset_of!(mdb_m4_cell, v_first) == 40);
const _: () = assert!(offset_of!(mdb_m4_cell, v_last) == 44);
const _: () = assert!(offset_of!(mdb_m4_cell, v_min) == 48);
const _: () = assert!(offset_of!(mdb_m4_cell, v_max) == 52);
const _: () = assert!(size_of::<mdb_moments_cell>() == 24);
const _: () = assert!(offset_of!(mdb_moments_cell, mean) == 8);
const _: () = assert!(offset_of!(mdb_moments_cell, m2) == 16);
const _: () = assert!(size_of::<mdb_comoments_cell>() == 48);
const _: () = assert!(offset_of!(mdb_comoments_cell, count) == 0);
const _: () = assert!(offset_of!(mdb_comoments_cell, mean_x) == 8);
const _: () = assert!(offset_of!(mdb_comoments_cell, mean_y) == 16);
const _: () = assert!(offset_of!(mdb_comoments_cell, m2_x) == 24);
const _: () = assert!(offset_of!(mdb_comoments_cell, m2_y) == 32);
const _: () = assert!(offset_of!(mdb_comoments_cell, c_xy) == 40);
const _: () = assert!(size_of::<mdb_derived_expr>() == 20);
const _: () = assert!(offset_of!(mdb_derived_expr, op) == 0);
const _: () = assert!(offset_of!(mdb_derived_expr, flags) == 4);
const _: () = assert!(offset_of!(mdb_derived_expr, a) == 8);
const _: () = assert!(offset_of!(mdb_derived_expr, b) == 12);
const _: () = assert!(offset_of!(mdb_derived_expr, c) == 16);
const _: () = assert!(size_of::<mdb_derived_cell>() == 32);
const _: () = assert!(offset_of!(mdb_derived_cell, count) == 0);
const _: () = assert!(offset_of!(mdb_derived_cell, mean) == 8);
const _: () = assert!(offset_of!(mdb_derived_cell, m2) == 16);
const _: () = assert!(offset_of!(mdb_derived_cell, min) == 24);
const _: () = assert!(offset_of!(mdb_derived_cell, max) == 28);
const _: () = assert!(size_of::<mdb_roll_request>() == 48);
const _: () = assert!(offset_of!(mdb_roll_request, kind) == 0);
const _: () = assert!(offset_of!(mdb_roll_request, flags) == 4);
const _: () = assert!(offset_of!(mdb_roll_request, n_outer) == 8);
const _: () = assert!(offset_of!(mdb_roll_request, n_buckets) == 16);
const _: () = assert!(offset_of!(mdb_roll_request, n_inner) == 24);
const _: () = assert!(offset_of!(mdb_roll_request, window) == 32);
const _: () = assert!(offset_of!(mdb_roll_request, stride) == 40);
