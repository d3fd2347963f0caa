//! Safe wrappers over `libmdb_hip.so` for the call sites of ModelarDB-RS that this library replaces
//! (see `rust/patches/`): `GridStream::poll_next` / `grid_and_append_to_leftovers_in_current_batch`
//! (crates/modelardb_storage/src/query/grid_exec.rs:261-429) through [`Context::grid_submit`] and
//! [`GridTicket::wait`]; the `Model*Accumulator::update_batch` methods
//! (crates/modelardb_storage/src/optimizer/model_simple_aggregates.rs:345-587) through
//! [`Context::aggregate`]; `try_compress_multivariate_time_series` and
//! `try_split_and_compress_univariate_time_series` (crates/modelardb_compression/src/compression.rs:42-179)
//! and `UncompressedDataManager::process_compressor_messages`
//! (crates/modelardb_server/src/storage/uncompressed_data_manager.rs:505-596) through
//! [`Context::compress_chunks`]: every series and field of a batch, or every finished ingest buffer of a
//! drained channel, in ONE launch per error bound (the fitter needs more than 10^4 chunks per launch to
//! beat one CPU thread; one launch per series does not).
//!
//! Every decision lives behind the C ABI; this crate only converts between Arrow arrays and the
//! pointer structs of `include/mdb_format.h`, owns the handles, and turns the `0 / 1 + last error`
//! convention into `Result`s. It copies no payload bytes on the way in.

pub mod sys;

use std::ffi::CStr;
use std::fmt::{Display, Formatter};
use std::iter;
use std::ptr::{self, NonNull};
use std::sync::Arc;

use arrow::array::{
    Array, ArrayRef, BinaryViewArray, Float32Array, Int8Array, Int16Array, StringViewArray,
};
use arrow::buffer::{BooleanBuffer, Buffer, ScalarBuffer};
use arrow::datatypes::Schema;
use arrow::record_batch::RecordBatch;
use modelardb_types::types::{ErrorBound, TimestampArray, ValueArray};

pub use sys::{
    mdb_agg_state as AggState, mdb_bucket_request as BucketRequest, mdb_grid_metrics as GridMetrics,
    mdb_comoments_cell as ComomentsCell, mdb_derived_cell as DerivedCell, mdb_derived_expr as DerivedExpr, mdb_hist_request as HistRequest, mdb_m4_cell as M4Cell,
    mdb_episode as Episode, mdb_episodes_request as EpisodesRequest, mdb_moments_cell as MomentsCell,
    mdb_integral_cell as IntegralCell, mdb_integral_request as IntegralRequest,
    mdb_sample_cell as SampleCell, mdb_sample_request as SampleRequest,
    mdb_change_cell as ChangeCell, mdb_change_request as ChangeRequest,
    mdb_dwell_request as DwellRequest,
    mdb_transit_request as TransitRequest,
    mdb_roll_request as RollRequest,
    mdb_value_filter as ValueFilter,
};
pub use sys::{MDB_INTEGRAL_LINEAR, MDB_INTEGRAL_STEP};
pub use sys::{MDB_SAMPLE_EXACT, MDB_SAMPLE_LINEAR, MDB_SAMPLE_STEP};
pub use sys::{MDB_CHANGE_INCREASE, MDB_CHANGE_NET, MDB_CHANGE_RATE, MDB_CHANGE_VARIATION};
pub use sys::MDB_DWELL_STEP;
pub use sys::{
    MDB_ROLL_AGG, MDB_ROLL_CHANGE, MDB_ROLL_COMOMENTS, MDB_ROLL_DERIVED, MDB_ROLL_INTEGRAL, MDB_ROLL_M4, MDB_ROLL_MOMENTS,
    MDB_ROLL_U64,
};
pub use sys::{MDB_HIST_MAX_EDGES, MDB_QUANTILE_BUCKETS_MAX_Q, MDB_QUANTILE_BUCKETS_PASSES};
pub use sys::{MDB_VALUE_HI_OPEN, MDB_VALUE_LO_OPEN, MDB_VALUE_NO_HI, MDB_VALUE_NO_LO};
pub use sys::{MDB_MASK_AND, MDB_MASK_ANDNOT, MDB_MASK_NOT, MDB_MASK_OR, MDB_MASK_XOR};
pub use sys::{MDB_AGG_AVG, MDB_AGG_COUNT, MDB_AGG_MAX, MDB_AGG_MIN, MDB_AGG_SUM};

/// Failure reported by the library (the text of `mdb_last_error()`).
#[derive(Debug, Clone)]
pub struct HipError(pub String);

impl Display for HipError {
    fn fmt(&self, f: &mut Formatter) -> std::fmt::Result {
        write!(f, "HIP Error: {}", self.0)
    }
}

impl std::error::Error for HipError {}

pub type Result<T> = std::result::Result<T, HipError>;

fn check(code: i32) -> Result<()> {
    if code == 0 {
        return Ok(());
    }
    // Valid until the next failing call on this thread (capi.rs:58-80 convention).
    let message = unsafe { CStr::from_ptr(sys::mdb_last_error()) };
    Err(HipError(message.to_string_lossy().into_owned()))
}

/// One `mdb_ctx`: a HIP stream plus the scratch memory the batches seen so far needed. Calls on one
/// context are serialised inside the library, so give every `GridStream`, accumulator and
/// compression thread its own.
pub struct Context(NonNull<sys::mdb_ctx>);

// The library locks the context's mutex in every entry point.
unsafe impl Send for Context {}
unsafe impl Sync for Context {}

impl Context {
    pub fn new(device: i32) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::mdb_init(device, &mut raw) })?;
        Ok(Self(NonNull::new(raw).expect("mdb_init returned success and a null context")))
    }

    fn raw(&self) -> *mut sys::mdb_ctx {
        self.0.as_ptr()
    }

    /// Give the grown scratch and staging memory back (call after an unusually large batch).
    pub fn trim(&self) -> Result<u64> {
        let mut released = 0u64;
        check(unsafe { sys::mdb_trim(self.raw(), &mut released) })?;
        Ok(released)
    }

    /// Device scratch beyond `bytes` is given back after every call on this context (0 keeps everything):
    /// for owners of many contexts, e.g. one `GridStream` per field column.
    pub fn set_scratch_limit(&self, bytes: u64) -> Result<()> {
        check(unsafe { sys::mdb_set_scratch_limit(self.raw(), bytes) })
    }

    /// `ncclCommInitRank` for the final aggregate merge; `unique_id` comes from
    /// [`comm_unique_id`] on one rank.
    pub fn comm_init(&self, rank: i32, world: i32, unique_id: &[u8; sys::MDB_COMM_ID_BYTES]) -> Result<()> {
        check(unsafe { sys::mdb_comm_init(self.raw(), rank, world, unique_id.as_ptr().cast()) })
    }

    /// Merge the partial aggregate states of all ranks (one 32-byte all-gather over RCCL and a fold
    /// in rank order, so every rank gets the same f64 sum, run after run).
    pub fn agg_all_reduce(&self, state: &mut AggState) -> Result<i32> {
        let mut ranks_seen = 0i32;
        check(unsafe { sys::mdb_agg_all_reduce(self.raw(), state, &mut ranks_seen) })?;
        Ok(ranks_seen)
    }
}

impl Drop for Context {
    fn drop(&mut self) {
        unsafe { sys::mdb_close(self.raw()) };
    }
}

pub fn comm_unique_id() -> Result<[u8; sys::MDB_COMM_ID_BYTES]> {
    let mut id = [0u8; sys::MDB_COMM_ID_BYTES];
    check(unsafe { sys::mdb_comm_unique_id(id.as_mut_ptr().cast()) })?;
    Ok(id)
}

impl From<ErrorBound> for sys::mdb_error_bound {
    fn from(error_bound: ErrorBound) -> Self {
        match error_bound {
            ErrorBound::Lossless => Self { kind: sys::MDB_EB_LOSSLESS, value: 0.0 },
            ErrorBound::Absolute(value) => Self { kind: sys::MDB_EB_ABSOLUTE, value },
            ErrorBound::Relative(value) => Self { kind: sys::MDB_EB_RELATIVE, value },
        }
    }
}

/// `modelardb_compression::is_value_within_error_bound` (models/mod.rs:53-77).
pub fn is_value_within_error_bound(error_bound: ErrorBound, real_value: f32, approximate_value: f32) -> bool {
    let mut within = 0i32;
    check(unsafe {
        sys::mdb_is_value_within_error_bound(error_bound.into(), real_value, approximate_value, &mut within)
    })
    .expect("a valid ErrorBound cannot be rejected");
    within != 0
}

/// `modelardb_compression::are_compressed_timestamps_regular` (models/timestamps.rs:199-202).
pub fn are_compressed_timestamps_regular(compressed_timestamps: &[u8]) -> bool {
    let mut regular = 0i32;
    check(unsafe {
        sys::mdb_are_compressed_timestamps_regular(
            compressed_timestamps.as_ptr(),
            compressed_timestamps.len() as u64,
            &mut regular,
        )
    })
    .expect("cannot fail for a slice");
    regular != 0
}

/// Borrowed `mdb_segments` view of the eight segment columns. Keeps the small pointer / size tables
/// the view refers to; the Arrow buffers themselves stay owned by the arrays.
pub struct SegmentsView<'a> {
    raw: sys::mdb_segments,
    _tables: Box<[(Vec<*const u8>, Vec<i64>); 3]>,
    _arrays: std::marker::PhantomData<&'a ()>,
}

impl<'a> SegmentsView<'a> {
    /// From the typed arrays `modelardb_types::arrays!` / `value!` yield (columns 0..=7 of
    /// `QUERY_COMPRESSED_SCHEMA`, crates/modelardb_types/src/schemas.rs:40-52).
    #[allow(clippy::too_many_arguments)]
    pub fn new(
        model_type_ids: &'a Int8Array,
        start_times: &'a TimestampArray,
        end_times: &'a TimestampArray,
        timestamps: &'a BinaryViewArray,
        min_values: &'a ValueArray,
        max_values: &'a ValueArray,
        values: &'a BinaryViewArray,
        residuals: &'a BinaryViewArray,
    ) -> Self {
        let mut tables: Box<[(Vec<*const u8>, Vec<i64>); 3]> = Box::default();
        let mut column = |index: usize, array: &BinaryViewArray| {
            let (pointers, sizes) = &mut tables[index];
            for buffer in array.data_buffers() {
                pointers.push(buffer.as_ptr());
                sizes.push(buffer.len() as i64);
            }
            sys::mdb_binview_col {
                views: array.views().as_ptr().cast(),
                buffers: pointers.as_ptr(),
                buffer_sizes: sizes.as_ptr(),
                n_buffers: pointers.len() as i32,
            }
        };
        let raw = sys::mdb_segments {
            n: model_type_ids.len() as u64,
            model_type_id: model_type_ids.values().as_ptr(),
            start_time: start_times.values().as_ptr(),
            end_time: end_times.values().as_ptr(),
            timestamps: column(0, timestamps),
            min_value: min_values.values().as_ptr(),
            max_value: max_values.values().as_ptr(),
            values: column(1, values),
            residuals: column(2, residuals),
        };
        Self { raw, _tables: tables, _arrays: std::marker::PhantomData }
    }

    /// From a batch whose first eight columns follow `QUERY_COMPRESSED_SCHEMA` (what `GridStream` and
    /// the accumulators are handed; tag columns may follow).
    pub fn from_record_batch(batch: &'a RecordBatch) -> Self {
        fn column<'b, T: 'static>(batch: &'b RecordBatch, index: usize) -> &'b T {
            batch
                .column(index)
                .as_any()
                .downcast_ref::<T>()
                .expect("The batch should follow QUERY_COMPRESSED_SCHEMA.")
        }
        Self::new(
            column::<Int8Array>(batch, 0),
            column::<TimestampArray>(batch, 1),
            column::<TimestampArray>(batch, 2),
            column::<BinaryViewArray>(batch, 3),
            column::<ValueArray>(batch, 4),
            column::<ValueArray>(batch, 5),
            column::<BinaryViewArray>(batch, 6),
            column::<BinaryViewArray>(batch, 7),
        )
    }
}

impl ValueFilter {
    /// Every value of every timestamp: narrow it with [`ValueFilter::time`], [`ValueFilter::above`] and
    /// [`ValueFilter::below`]. For `WHERE field op literal` the caller converts the literal to the f32 bound that
    /// selects the same f32 values (the Python binding's `value_filter` does so exactly, NaN and ±0 included).
    pub fn all() -> Self {
        ValueFilter {
            t_lo: i64::MIN,
            t_hi: i64::MAX,
            v_lo: 0.0,
            v_hi: 0.0,
            flags: MDB_VALUE_NO_LO | MDB_VALUE_NO_HI,
            reserved: 0,
        }
    }

    /// ANDs `t_lo <= timestamp <= t_hi`.
    pub fn time(mut self, t_lo: i64, t_hi: i64) -> Self {
        self.t_lo = t_lo;
        self.t_hi = t_hi;
        self
    }

    /// `value >= v_lo` (`open`: `value > v_lo`), in totalOrder.
    pub fn above(mut self, v_lo: f32, open: bool) -> Self {
        self.v_lo = v_lo;
        self.flags &= !(MDB_VALUE_NO_LO | MDB_VALUE_LO_OPEN);
        if open {
            self.flags |= MDB_VALUE_LO_OPEN;
        }
        self
    }

    /// `value <= v_hi` (`open`: `value < v_hi`), in totalOrder.
    pub fn below(mut self, v_hi: f32, open: bool) -> Self {
        self.v_hi = v_hi;
        self.flags &= !(MDB_VALUE_NO_HI | MDB_VALUE_HI_OPEN);
        if open {
            self.flags |= MDB_VALUE_HI_OPEN;
        }
        self
    }
}

/// The block of page-locked memory `mdb_grid_batch_owned` reconstructed a batch into. Arrow buffers
/// made from it keep it alive; the last one to go returns it to the library's pool.
struct GridBlock(NonNull<sys::mdb_grid_result>);

unsafe impl Send for GridBlock {}
unsafe impl Sync for GridBlock {}
impl std::panic::RefUnwindSafe for GridBlock {}

impl Drop for GridBlock {
    fn drop(&mut self) {
        unsafe { sys::mdb_grid_result_free(self.0.as_ptr()) };
    }
}

/// What one call of [`Context::grid`] produced.
pub struct GridOutput {
    /// `leftovers.len() + rows created` timestamps: the leftovers first (grid_exec.rs:302-320).
    pub timestamps: TimestampArray,
    pub values: ValueArray,
    /// Data points each segment row reconstructed to, for the tag replication of grid_exec.rs:341-346.
    pub rows_per_segment: Vec<u32>,
    pub metrics: GridMetrics,
}

/// The arrays of an owned grid result (`mdb_grid_batch_owned` / `mdb_grid_batch_filter_owned`), the leftovers copied
/// into the room in front of the new points.
fn grid_output(raw: *mut sys::mdb_grid_result, leftover_timestamps: &[i64], leftover_values: &[f32]) -> GridOutput {
    let leftovers = leftover_timestamps.len();
    let block = Arc::new(GridBlock(NonNull::new(raw).expect("success with a null result")));
    let result = unsafe { block.0.as_ref() };
    let total = leftovers + result.n as usize;
    let rows_per_segment =
        unsafe { std::slice::from_raw_parts(result.rows_per_segment, result.n_segments as usize) }.to_vec();
    let (timestamps, values) = unsafe {
        // `reserve_front` rows of writable room sit in front of the new points.
        let first_timestamp = result.timestamps.sub(leftovers);
        let first_value = result.values.sub(leftovers);
        ptr::copy_nonoverlapping(leftover_timestamps.as_ptr(), first_timestamp, leftovers);
        ptr::copy_nonoverlapping(leftover_values.as_ptr(), first_value, leftovers);
        let timestamps = Buffer::from_custom_allocation(
            NonNull::new_unchecked(first_timestamp.cast::<u8>()),
            8 * total,
            block.clone(),
        );
        let values =
            Buffer::from_custom_allocation(NonNull::new_unchecked(first_value.cast::<u8>()), 4 * total, block.clone());
        (timestamps, values)
    };
    GridOutput {
        timestamps: TimestampArray::new(ScalarBuffer::new(timestamps, 0, total), None),
        values: ValueArray::new(ScalarBuffer::new(values, 0, total), None),
        rows_per_segment,
        metrics: result.metrics,
    }
}

/// `states` of a bucket call must hold exactly `n_groups * n_buckets` cells.
fn check_bucket_cells(request: &BucketRequest, n_states: usize) -> Result<()> {
    let cells = (request.n_groups as u64).checked_mul(request.n_buckets);
    if cells != Some(n_states as u64) {
        return Err(HipError(format!(
            "states holds {} cells, the request n_groups * n_buckets = {} * {}",
            n_states, request.n_groups, request.n_buckets
        )));
    }
    Ok(())
}

/// `into[j]` merged with `from[j]` by the four rules of [`Context::m4_buckets`] (host arithmetic, no GPU).
pub fn m4_merge(into: &mut [M4Cell], from: &[M4Cell]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} cells merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_m4_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// `into[j]` merged with `from[j]` by the merge rule of [`Context::moments_buckets`] (host arithmetic, no GPU): what
/// a `VarianceAccumulator`-shaped accumulator does in `merge_batch`.
pub fn moments_merge(into: &mut [MomentsCell], from: &[MomentsCell]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} cells merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_moments_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// `into[j]` merged with `from[j]` by the merge rule of [`Context::comoments_buckets`] (host arithmetic, no GPU): what
/// a `CovarianceAccumulator`-shaped accumulator does in `merge_batch`.
pub fn comoments_merge(into: &mut [ComomentsCell], from: &[ComomentsCell]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} cells merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_comoments_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// The `(count, mean, m2)` of the x field (`which` 0) or the y field (1) of every cell: what [`moments_variance`]
/// takes (host arithmetic, no GPU).
pub fn comoments_moments(cells: &[ComomentsCell], which: u32) -> Result<Vec<MomentsCell>> {
    let mut out = vec![MomentsCell::default(); cells.len()];
    check(unsafe { sys::mdb_comoments_moments(cells.as_ptr(), cells.len() as u64, which, out.as_mut_ptr()) })?;
    Ok(out)
}

/// The statistic `kind` (`sys::MDB_COMOMENTS_*`) per cell (host arithmetic, no GPU): `covar_pop`, `covar_samp`,
/// `corr`, `regr_slope`, `regr_intercept`, `regr_r2` - the `regr_*` with x as the independent variable, SQL's
/// `regr_*(y, x)`; NaN where the cell does not allow it.
pub fn comoments_finish(cells: &[ComomentsCell], kind: u32) -> Result<Vec<f64>> {
    let mut out = vec![0.0f64; cells.len()];
    check(unsafe { sys::mdb_comoments_finish(cells.as_ptr(), cells.len() as u64, kind, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `z[j] = f(x[j], y[j])` by the evaluator the kernels of [`Context::derived_buckets`] use (host arithmetic, no GPU):
/// binary32 operations in the written order, nothing fused.
pub fn derived_apply(expr: &DerivedExpr, x: &[f32], y: &[f32]) -> Result<Vec<f32>> {
    if x.len() != y.len() {
        return Err(HipError(format!("{} values of x against {} of y", x.len(), y.len())));
    }
    let mut z = vec![0.0f32; x.len()];
    check(unsafe { sys::mdb_derived_apply(expr, x.as_ptr(), y.as_ptr(), x.len() as u64, z.as_mut_ptr()) })?;
    Ok(z)
}

/// `into[j]` merged with `from[j]` by the merge rule of [`Context::derived_buckets`] (host arithmetic, no GPU).
pub fn derived_merge(into: &mut [DerivedCell], from: &[DerivedCell]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} cells merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_derived_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// The `(count, mean, m2)` of every cell: what [`moments_variance`] takes (host arithmetic, no GPU).
pub fn derived_stats(cells: &[DerivedCell]) -> Result<Vec<MomentsCell>> {
    let mut out = vec![MomentsCell::default(); cells.len()];
    check(unsafe { sys::mdb_derived_stats(cells.as_ptr(), cells.len() as u64, out.as_mut_ptr()) })?;
    Ok(out)
}

/// A cell type that [`roll_cells`] can roll: its `MDB_ROLL_*` kind names the merge rule.
pub trait RollCell: Copy {
    const KIND: u32;
}
impl RollCell for AggState {
    const KIND: u32 = MDB_ROLL_AGG;
}
impl RollCell for M4Cell {
    const KIND: u32 = MDB_ROLL_M4;
}
/// (also the cells of `mdb_binned_buckets*`)
impl RollCell for MomentsCell {
    const KIND: u32 = MDB_ROLL_MOMENTS;
}
/// (also the cells of `mdb_trend_buckets*`)
impl RollCell for ComomentsCell {
    const KIND: u32 = MDB_ROLL_COMOMENTS;
}
impl RollCell for DerivedCell {
    const KIND: u32 = MDB_ROLL_DERIVED;
}
impl RollCell for IntegralCell {
    const KIND: u32 = MDB_ROLL_INTEGRAL;
}
impl RollCell for ChangeCell {
    const KIND: u32 = MDB_ROLL_CHANGE;
}
/// The counters of `mdb_hist_buckets*`, `mdb_dwell_buckets*` and `mdb_transit_buckets*`: wrapping add.
impl RollCell for u64 {
    const KIND: u32 = MDB_ROLL_U64;
}

/// The number of whole windows of `window` buckets every `stride` buckets in `n_buckets` buckets (host arithmetic).
pub fn roll_windows(n_buckets: u64, window: u64, stride: u64) -> Result<u64> {
    let request = RollRequest { kind: MDB_ROLL_U64, flags: 0, n_outer: 1, n_buckets, n_inner: 1, window, stride };
    let mut n_windows = 0u64;
    check(unsafe { sys::mdb_roll_windows(&request, &mut n_windows) })?;
    Ok(n_windows)
}

/// Rolling windows over the cells of a per-bucket operator (host arithmetic, no GPU): `cells` is row-major
/// `[n_outer][n_buckets][n_inner]`, the result `[n_outer][n_windows][n_inner]`; window `k` is the merge of the buckets
/// `[k * stride, k * stride + window)` by the operator's merge rule, in the fixed order `mdb.h` states.
pub fn roll_cells<C: RollCell>(cells: &[C], n_outer: u64, n_buckets: u64, n_inner: u64, window: u64, stride: u64)
                               -> Result<Vec<C>> {
    let request = RollRequest { kind: C::KIND, flags: 0, n_outer, n_buckets, n_inner, window, stride };
    let n_windows = roll_windows(n_buckets, window, stride)?;
    let expected = n_outer.checked_mul(n_buckets).and_then(|n| n.checked_mul(n_inner));
    if expected != Some(cells.len() as u64) {
        return Err(HipError(format!("{} cells for [{n_outer}][{n_buckets}][{n_inner}]", cells.len())));
    }
    let n_out = (n_outer * n_windows * n_inner) as usize;
    if n_out == 0 {
        return Ok(Vec::new());
    }
    let mut out = vec![cells[0]; n_out];
    check(unsafe { sys::mdb_roll_cells(&request, cells.as_ptr().cast(), out.as_mut_ptr().cast(), n_out as u64) })?;
    Ok(out)
}

/// `into[k] += from[k]`, both members: the merge of `mdb_integral_buckets*` (host arithmetic, no GPU).
pub fn integral_merge(into: &mut [IntegralCell], from: &[IntegralCell]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} cells merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_integral_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// `into[k]` merged with `from[k]`: a cell with `count == 0` takes the other whole, else both members are added - the
/// merge of `mdb_sample_at*` (host arithmetic, no GPU).
pub fn sample_merge(into: &mut [SampleCell], from: &[SampleCell]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} cells merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_sample_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// The sampled value `sum / count` per cell, NaN where `count == 0`: the gaps of gap-fill (host arithmetic, no GPU).
pub fn sample_values(cells: &[SampleCell]) -> Result<Vec<f64>> {
    let mut out = vec![0.0f64; cells.len()];
    check(unsafe { sys::mdb_sample_values(cells.as_ptr(), cells.len() as u64, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `into[k]` merged with `from[k]`: the integers and the sums added, the larger of each maximum - the merge of
/// `mdb_change_buckets*` (host arithmetic, no GPU).
pub fn change_merge(into: &mut [ChangeCell], from: &[ChangeCell]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} cells merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_change_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// One figure per cell (host arithmetic, no GPU): `MDB_CHANGE_NET` `rise - fall`, `MDB_CHANGE_VARIATION`
/// `rise + fall`, `MDB_CHANGE_INCREASE` `rise + reset_sum`, `MDB_CHANGE_RATE` the increase per second; NaN where
/// `count == 0` (`MDB_CHANGE_RATE`: or `duration == 0`).
pub fn change_finish(cells: &[ChangeCell], kind: u32) -> Result<Vec<f64>> {
    let mut out = vec![0.0f64; cells.len()];
    check(unsafe { sys::mdb_change_finish(cells.as_ptr(), cells.len() as u64, kind, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `into[k] += from[k]`: the merge of two counter arrays of `mdb_dwell_buckets*` (host arithmetic, no GPU).
pub fn dwell_merge(into: &mut [u64], from: &[u64]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} counters merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_dwell_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// The share of its (group, bucket) row's linked time each cell holds: `dwell / sum over the row's n_cells cells`, NaN
/// where that sum is 0 (host arithmetic, no GPU). `dwell.len()` must be a multiple of `n_cells`.
pub fn dwell_share(dwell: &[u64], n_cells: u32) -> Result<Vec<f64>> {
    if n_cells == 0 || dwell.len() % n_cells as usize != 0 {
        return Err(HipError(format!("{} counters are no whole number of rows of {} cells", dwell.len(), n_cells)));
    }
    let mut out = vec![0.0f64; dwell.len()];
    check(unsafe { sys::mdb_dwell_share(dwell.as_ptr(), (dwell.len() / n_cells as usize) as u64, n_cells, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `into[k] += from[k]`: the merge of two counter arrays of `mdb_transit_buckets*` (host arithmetic, no GPU).
pub fn transit_merge(into: &mut [u64], from: &[u64]) -> Result<()> {
    if into.len() != from.len() {
        return Err(HipError(format!("{} counters merged into {}", from.len(), into.len())));
    }
    check(unsafe { sys::mdb_transit_merge_n(into.as_mut_ptr(), from.as_ptr(), into.len() as u64) })
}

/// The pairs that went over each edge, per (group, bucket) row of `n_cells * n_cells` counters `[from][to]`: returns
/// `(up, down)` with `n_cells - 1` entries per row, `up[e]` the sum of `counts[from <= e < to]` and `down[e]` the sum of
/// `counts[to <= e < from]` (host arithmetic, no GPU). `counts.len()` must be a multiple of `n_cells * n_cells`.
pub fn transit_crossings(counts: &[u64], n_cells: u32) -> Result<(Vec<u64>, Vec<u64>)> {
    let matrix = n_cells as usize * n_cells as usize;
    if n_cells == 0 || counts.len() % matrix != 0 {
        return Err(HipError(format!("{} counters are no whole number of matrices of {} x {} cells", counts.len(), n_cells, n_cells)));
    }
    let n_rows = counts.len() / matrix;
    let mut up = vec![0u64; n_rows * (n_cells as usize - 1)];
    let mut down = vec![0u64; n_rows * (n_cells as usize - 1)];
    check(unsafe { sys::mdb_transit_crossings(counts.as_ptr(), n_rows as u64, n_cells, up.as_mut_ptr(), down.as_mut_ptr()) })?;
    Ok((up, down))
}

// The counters of mdb_transit_buckets*: n_groups * n_buckets matrices of (edges + 1)^2.
fn check_transit_counts(request: &BucketRequest, n_edges: usize, n_counts: usize) -> Result<()> {
    let n_cells = n_edges as u64 + 1;
    check_hist_bucket_cells(request, n_cells.saturating_mul(n_cells), n_counts)
}

/// The time-weighted average `integral / duration` per cell, NaN where `duration == 0` (host arithmetic, no GPU).
pub fn integral_average(cells: &[IntegralCell]) -> Result<Vec<f64>> {
    let mut out = vec![0.0f64; cells.len()];
    check(unsafe { sys::mdb_integral_average(cells.as_ptr(), cells.len() as u64, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `m2 / (count - ddof)` per cell (host arithmetic, no GPU): `ddof` 0 is `var_pop`, 1 `var_samp`; NaN where the count
/// does not allow it. The standard deviation is its `sqrt`.
pub fn moments_variance(cells: &[MomentsCell], ddof: u32) -> Result<Vec<f64>> {
    let mut variance = vec![0.0f64; cells.len()];
    check(unsafe { sys::mdb_moments_variance(cells.as_ptr(), cells.len() as u64, ddof, variance.as_mut_ptr()) })?;
    Ok(variance)
}

/// The cells of a histogram call: `counts` is row-major `[n_groups][edges + 1]`.
fn check_hist_cells(n_groups: u32, edges: &[f32], n_counts: usize) -> Result<()> {
    if (n_groups as u64) * (edges.len() as u64 + 1) != n_counts as u64 {
        return Err(HipError(format!(
            "counts holds {} cells, the request n_groups * (edges + 1) = {} * {}",
            n_counts, n_groups, edges.len() + 1
        )));
    }
    Ok(())
}

/// The cells of a per-bucket histogram call: `counts` is row-major `[n_groups][n_buckets][n_cells]`.
fn check_hist_bucket_cells(request: &BucketRequest, n_cells: u64, n_counts: usize) -> Result<()> {
    let wanted = (request.n_groups as u64).checked_mul(request.n_buckets).and_then(|rows| rows.checked_mul(n_cells));
    if wanted != Some(n_counts as u64) {
        return Err(HipError(format!(
            "counts holds {} cells, the request n_groups * n_buckets * (edges + 1) = {} * {} * {}",
            n_counts, request.n_groups, request.n_buckets, n_cells
        )));
    }
    Ok(())
}

fn hist_request(edges: &[f32], n_groups: u32, time_range: Option<(i64, i64)>) -> HistRequest {
    let (t_lo, t_hi) = time_range.unwrap_or((i64::MIN, i64::MAX));
    // (more edges than a u32 holds are more than MDB_HIST_MAX_EDGES: the library says so)
    HistRequest { t_lo, t_hi, n_edges: u32::try_from(edges.len()).unwrap_or(u32::MAX), n_groups, flags: 0, reserved: 0 }
}

/// The cell of `value` under `edges`: the number of edges at or below it in totalOrder (host arithmetic, no GPU).
/// Fails for edges `Context::hist` would reject.
pub fn hist_cell_of(edges: &[f32], value: f32) -> Result<u32> {
    let mut cell = 0u32;
    let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
    check(unsafe { sys::mdb_hist_cell_of(edges.as_ptr(), n_edges, value, &mut cell) })?;
    Ok(cell)
}

/// `(rank_lo, rank_hi, fraction)` of quantile `q` over `n_points` points: p = q * (n_points - 1), its floor, its ceil
/// and p - floor(p) (host arithmetic, no GPU). `percentile_cont` is `lo + (hi - lo) * fraction`.
pub fn quantile_positions(q: f64, n_points: u64) -> Result<(u64, u64, f64)> {
    let (mut rank_lo, mut rank_hi, mut fraction) = (0u64, 0u64, 0f64);
    check(unsafe { sys::mdb_quantile_positions(q, n_points, &mut rank_lo, &mut rank_hi, &mut fraction) })?;
    Ok((rank_lo, rank_hi, fraction))
}

/// Group ids of a bucket call: one per segment row, if given.
/// Copies the episodes of a result out and frees it.
fn take_episodes(out: *mut sys::mdb_episodes_result) -> (Vec<Episode>, u64, u64) {
    let result = unsafe { &*out };
    let episodes = if result.n == 0 {
        Vec::new()
    } else {
        unsafe { std::slice::from_raw_parts(result.episodes, result.n as usize) }.to_vec()
    };
    let counts = (result.n_rows, result.n_passing);
    unsafe { sys::mdb_episodes_result_free(out) };
    (episodes, counts.0, counts.1)
}

fn check_group_ids(segments: &SegmentsView, group_of_segment: Option<&[u32]>) -> Result<()> {
    if let Some(groups) = group_of_segment {
        if groups.len() as u64 != segments.raw.n {
            return Err(HipError(format!("{} group ids for {} segments", groups.len(), segments.raw.n)));
        }
    }
    Ok(())
}

impl Context {
    /// Replaces the per-row `modelardb_compression::grid` loop of grid_exec.rs:323-356 for a whole
    /// batch: one upload of the segment columns, the kernels, one copy of the reconstructed columns
    /// into page-locked memory, which the returned arrays wrap without copying. `leftover_*` are the
    /// rows of the current batch that have not been handed out yet; they are placed in front.
    /// `time_range`: `Some((lo, hi))` reconstructs only `lo <= timestamp <= hi`.
    pub fn grid(
        &self,
        segments: &SegmentsView,
        leftover_timestamps: &[i64],
        leftover_values: &[f32],
        time_range: Option<(i64, i64)>,
    ) -> Result<GridOutput> {
        assert_eq!(leftover_timestamps.len(), leftover_values.len());
        let leftovers = leftover_timestamps.len();
        let (flags, t_lo, t_hi) = match time_range {
            Some((lo, hi)) => (sys::MDB_GRID_HAS_RANGE, lo, hi),
            None => (0, 0, 0),
        };
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::mdb_grid_batch_owned(self.raw(), &segments.raw, flags, t_lo, t_hi, leftovers as u64, &mut raw)
        })?;
        Ok(grid_output(raw, leftover_timestamps, leftover_values))
    }

    /// [`Context::grid`] with a value predicate and a time range pushed down (`mdb_grid_batch_filter_owned`):
    /// replaces GridExec -> FilterExec (grid_exec.rs:366-387 and the FilterExec DataFusion keeps above it for a
    /// predicate on the field column). Only the passing rows cross PCIe; `rows_per_segment` counts them per segment.
    pub fn grid_filter_owned(
        &self,
        segments: &SegmentsView,
        filter: &ValueFilter,
        leftover_timestamps: &[i64],
        leftover_values: &[f32],
    ) -> Result<GridOutput> {
        assert_eq!(leftover_timestamps.len(), leftover_values.len());
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::mdb_grid_batch_filter_owned(self.raw(), &segments.raw, filter, leftover_timestamps.len() as u64, &mut raw)
        })?;
        Ok(grid_output(raw, leftover_timestamps, leftover_values))
    }

    /// COUNT / MIN / MAX / SUM of the points that pass `filter`, folded into `state` without materialising a data
    /// point: replaces GridExec -> FilterExec -> AggregateExec.
    pub fn agg_filter(
        &self,
        segments: &SegmentsView,
        filter: &ValueFilter,
        which_mask: u32,
        state: &mut AggState,
    ) -> Result<()> {
        check(unsafe { sys::mdb_agg_batch_filter(self.raw(), &segments.raw, filter, which_mask, state) })
    }

    /// [`Context::agg_filter`] for several batches at once (rows in the order of the slice), folded as one batch.
    pub fn agg_filter_list(
        &self,
        segments: &[SegmentsView],
        filter: &ValueFilter,
        which_mask: u32,
        state: &mut AggState,
    ) -> Result<()> {
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_agg_batch_filter_list(self.raw(), inputs.as_ptr(), inputs.len() as u32, filter, which_mask, state)
        })
    }

    /// `agg(target) WHERE filters[0](pred_fields[0]) AND filters[1](pred_fields[1]) ...` (`mdb_agg_batch_where`):
    /// replaces GridExec per field -> SortedJoinExec -> FilterExec -> AggregateExec when every conjunct of the
    /// FilterExec compares ONE field column (or the timestamp) with literals. The time range of the call is the
    /// intersection of the filters' ranges; the field batches must line up (the same series in the same order with
    /// the same timestamps - the fields of one time series table do). `target` may be one of `pred_fields`.
    pub fn agg_where(
        &self,
        pred_fields: &[&SegmentsView],
        filters: &[ValueFilter],
        target: &SegmentsView,
        which_mask: u32,
        state: &mut AggState,
    ) -> Result<()> {
        assert_eq!(pred_fields.len(), filters.len());
        let inputs: Vec<*const sys::mdb_segments> = pred_fields.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_agg_batch_where(self.raw(), inputs.as_ptr(), filters.as_ptr(), inputs.len() as u32, &target.raw,
                                     which_mask, state)
        })
    }

    /// The rows of `target` under the same conjunction (`mdb_grid_batch_where_owned`), timestamps and values: what
    /// the first field column of the join contributes. Only the selected rows cross PCIe.
    pub fn grid_where_owned(
        &self,
        pred_fields: &[&SegmentsView],
        filters: &[ValueFilter],
        target: &SegmentsView,
        leftover_timestamps: &[i64],
        leftover_values: &[f32],
    ) -> Result<GridOutput> {
        assert_eq!(pred_fields.len(), filters.len());
        assert_eq!(leftover_timestamps.len(), leftover_values.len());
        let inputs: Vec<*const sys::mdb_segments> = pred_fields.iter().map(|view| &view.raw as *const _).collect();
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::mdb_grid_batch_where_owned(self.raw(), inputs.as_ptr(), filters.as_ptr(), inputs.len() as u32,
                                            &target.raw, 0, leftover_timestamps.len() as u64, &mut raw)
        })?;
        Ok(grid_output(raw, leftover_timestamps, leftover_values))
    }

    /// The same with `MDB_GRID_VALUES_ONLY`: the values of the selected rows alone, for the second and later field
    /// columns of the join (sorted_join_exec.rs:268-275 takes the timestamps from the first input).
    pub fn grid_where_values_owned(
        &self,
        pred_fields: &[&SegmentsView],
        filters: &[ValueFilter],
        target: &SegmentsView,
    ) -> Result<(ValueArray, Vec<u32>)> {
        assert_eq!(pred_fields.len(), filters.len());
        let inputs: Vec<*const sys::mdb_segments> = pred_fields.iter().map(|view| &view.raw as *const _).collect();
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::mdb_grid_batch_where_owned(self.raw(), inputs.as_ptr(), filters.as_ptr(), inputs.len() as u32,
                                            &target.raw, sys::MDB_GRID_VALUES_ONLY, 0, &mut raw)
        })?;
        let block = Arc::new(GridBlock(NonNull::new(raw).expect("success with a null result")));
        let result = unsafe { block.0.as_ref() };
        let total = result.n as usize;
        let rows_per_segment =
            unsafe { std::slice::from_raw_parts(result.rows_per_segment, result.n_segments as usize) }.to_vec();
        let values = unsafe {
            Buffer::from_custom_allocation(NonNull::new_unchecked(result.values.cast::<u8>()), 4 * total, block.clone())
        };
        Ok((ValueArray::new(ScalarBuffer::new(values, 0, total), None), rows_per_segment))
    }

    /// Device memory for a row mask over `n_rows` rows (`ceil(n_rows / 64)` words, not cleared: every call that
    /// writes a mask writes all of its words).
    pub fn row_mask(&self, n_rows: u64) -> Result<RowMask<'_>> {
        let mut words = ptr::null_mut();
        check(unsafe { sys::mdb_dev_alloc(self.raw(), n_rows.div_ceil(64).max(1) * 8, &mut words) })?;
        Ok(RowMask { context: self, words: words.cast(), n_rows, cap_words: n_rows.div_ceil(64).max(1) })
    }

    /// Replaces the per-row `len` / `sum` loops of the accumulators: folds the batch into `state`
    /// for the aggregates in `which_mask` (`MDB_AGG_*`).
    pub fn aggregate(&self, segments: &SegmentsView, which_mask: u32, state: &mut AggState) -> Result<()> {
        check(unsafe { sys::mdb_agg_batch(self.raw(), &segments.raw, which_mask, state) })
    }

    /// The same for several batches at once (rows in the order of the slice): uploaded and reduced as ONE
    /// batch, so that accumulators which are handed 8192 segments at a time can fold hundreds of
    /// thousands with one call (patches/0002-model_simple_aggregates.patch: `PendingSegments`).
    pub fn aggregate_list(&self, segments: &[SegmentsView], which_mask: u32, state: &mut AggState) -> Result<()> {
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe { sys::mdb_agg_batch_list(self.raw(), inputs.as_ptr(), inputs.len() as u32, which_mask, state) })
    }

    /// The same restricted to `t_lo <= timestamp <= t_hi`, without materialising a data point.
    pub fn aggregate_range(
        &self,
        segments: &SegmentsView,
        t_lo: i64,
        t_hi: i64,
        which_mask: u32,
        state: &mut AggState,
    ) -> Result<()> {
        check(unsafe { sys::mdb_agg_batch_range(self.raw(), &segments.raw, t_lo, t_hi, which_mask, state) })
    }

    /// [`Context::aggregate_list`] restricted to `t_lo <= timestamp <= t_hi`: what the accumulators of a query
    /// with a range on the timestamp fold their pending batches with
    /// (patches/0002-model_simple_aggregates.patch: `PendingSegments::fold_into`).
    pub fn aggregate_range_list(
        &self,
        segments: &[SegmentsView],
        t_lo: i64,
        t_hi: i64,
        which_mask: u32,
        state: &mut AggState,
    ) -> Result<()> {
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_agg_batch_range_list(self.raw(), inputs.as_ptr(), inputs.len() as u32, t_lo, t_hi, which_mask, state)
        })
    }

    /// COUNT / MIN / MAX / SUM per bucket of `date_bin(width, ts, origin)` and group, without materialising a data
    /// point: `states` is row-major `[n_groups][n_buckets]`, each cell folded like `mdb_agg_merge` (a cell without
    /// points stays as it was). `group_of_segment`: one id per segment row (`None`: all in group 0).
    pub fn agg_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &BucketRequest,
        states: &mut [AggState],
    ) -> Result<()> {
        check_bucket_cells(request, states.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_agg_buckets(self.raw(), &segments.raw, groups, request, states.as_mut_ptr()) })
    }

    /// [`Context::agg_buckets`] of the points that pass `filter` (its time range ANDed with the request's): replaces
    /// GridExec -> FilterExec -> AggregateExec under `GROUP BY <tags>, date_bin(...)`. A cell without a passing
    /// point stays as it was.
    pub fn agg_buckets_filter(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &BucketRequest,
        filter: &ValueFilter,
        states: &mut [AggState],
    ) -> Result<()> {
        check_bucket_cells(request, states.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe {
            sys::mdb_agg_buckets_filter(self.raw(), &segments.raw, groups, request, filter, states.as_mut_ptr())
        })
    }

    /// [`Context::agg_buckets_filter`] for several batches at once (rows in the order of the slice), folded as one
    /// batch. `group_of_segment`: `None`, or one entry per batch (`None`: that batch's rows in group 0).
    pub fn agg_buckets_filter_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &BucketRequest,
        filter: &ValueFilter,
        states: &mut [AggState],
    ) -> Result<()> {
        check_bucket_cells(request, states.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_agg_buckets_filter_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                             request, filter, states.as_mut_ptr())
        })
    }

    /// M4 downsampling: per bucket of `date_bin(width, ts, origin)` and group the first, last, lowest and highest data
    /// point with their timestamps, and the count, without materialising a data point. `cells` is row-major
    /// `[n_groups][n_buckets]` (fresh: `M4Cell::default()`); the batch is merged into it by rules that depend on
    /// nothing but the set of points, and a cell without points stays as it was. `request.which_mask` must be 0.
    pub fn m4_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &BucketRequest,
        cells: &mut [M4Cell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_m4_buckets(self.raw(), &segments.raw, groups, request, cells.as_mut_ptr()) })
    }

    /// [`Context::m4_buckets`] for several batches at once (rows in the order of the slice), merged as one batch.
    /// `group_of_segment`: `None`, or one entry per batch (`None`: that batch's rows in group 0).
    pub fn m4_buckets_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &BucketRequest,
        cells: &mut [M4Cell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_m4_buckets_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32, request,
                                     cells.as_mut_ptr())
        })
    }

    /// Variance and standard deviation: per bucket of `date_bin(width, ts, origin)` and group the count, the mean and
    /// `m2`, the sum of `(v - mean)^2`, without materialising a data point. `cells` is row-major `[n_groups][n_buckets]`
    /// (fresh: `MomentsCell::default()`); the batch is merged into it, and a cell without points stays as it was.
    /// `request.which_mask` must be 0. [`moments_variance`] turns cells into variances.
    pub fn moments_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &BucketRequest,
        cells: &mut [MomentsCell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_moments_buckets(self.raw(), &segments.raw, groups, request, cells.as_mut_ptr()) })
    }

    /// [`Context::moments_buckets`] for several batches at once (rows in the order of the slice), merged as one batch.
    /// `group_of_segment`: `None`, or one entry per batch (`None`: that batch's rows in group 0).
    pub fn moments_buckets_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &BucketRequest,
        cells: &mut [MomentsCell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_moments_buckets_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                          request, cells.as_mut_ptr())
        })
    }

    /// Covariance and correlation of two fields: per bucket of `date_bin(width, ts, origin)` and group the count, both
    /// means, both `m2` and `c_xy` of the pairs `(x, y)`. `x` and `y` are two field columns of the same series that
    /// line up row for row under the request's time range (only the row count is checked); `x` is walked on its
    /// segments, `y` is rebuilt values-only into device scratch (4 B per row, never copied to the host). `cells` is
    /// row-major `[n_groups][n_buckets]` (fresh: `ComomentsCell::default()`); the batches are merged into it, and a
    /// cell without pairs stays as it was. `group_of_segment_x` is per segment of `x`; `request.which_mask` must be 0.
    /// [`comoments_finish`] turns cells into `corr` / `covar_*` / `regr_*`.
    pub fn comoments_buckets(
        &self,
        x: &SegmentsView,
        y: &SegmentsView,
        group_of_segment_x: Option<&[u32]>,
        request: &BucketRequest,
        cells: &mut [ComomentsCell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        check_group_ids(x, group_of_segment_x)?;
        let groups = group_of_segment_x.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_comoments_buckets(self.raw(), &x.raw, &y.raw, groups, request, cells.as_mut_ptr()) })
    }

    /// [`Context::comoments_buckets`] for several batches per field (rows in the order of each slice), merged as one
    /// batch per field: the cuts of `xs` and `ys` need not coincide. `group_of_segment_x`: `None`, or one entry per
    /// batch of `xs` (`None`: that batch's rows in group 0).
    pub fn comoments_buckets_list(
        &self,
        xs: &[SegmentsView],
        ys: &[SegmentsView],
        group_of_segment_x: Option<&[Option<&[u32]>]>,
        request: &BucketRequest,
        cells: &mut [ComomentsCell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        if let Some(groups) = group_of_segment_x {
            if groups.len() != xs.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), xs.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(xs.len());
        for (k, view) in xs.iter().enumerate() {
            let groups = group_of_segment_x.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let x_inputs: Vec<*const sys::mdb_segments> = xs.iter().map(|view| &view.raw as *const _).collect();
        let y_inputs: Vec<*const sys::mdb_segments> = ys.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_comoments_buckets_list(self.raw(), x_inputs.as_ptr(), x_inputs.len() as u32, y_inputs.as_ptr(),
                                            y_inputs.len() as u32, group_pointers.as_ptr(), request, cells.as_mut_ptr())
        })
    }

    /// The generated column `z = f(x, y)` of two fields that line up row for row under `[t_lo, t_hi]` (only the row
    /// count is checked): where a `GeneratedAsExec` over a `SortedJoinExec` of two fields rebuilds every point of both
    /// on the host. Returns the timestamps of `x` and `z`.
    pub fn derived_values(
        &self,
        x: &SegmentsView,
        y: &SegmentsView,
        expr: &DerivedExpr,
        t_lo: i64,
        t_hi: i64,
    ) -> Result<(Vec<i64>, Vec<f32>)> {
        let mut rows = 0u64;
        check(unsafe { sys::mdb_grid_count_range(self.raw(), &x.raw, t_lo, t_hi, &mut rows) })?;
        let mut timestamps = vec![0i64; rows as usize];
        let mut values = vec![0.0f32; rows as usize];
        check(unsafe {
            sys::mdb_derived_values(self.raw(), &x.raw, &y.raw, expr, t_lo, t_hi, timestamps.as_mut_ptr(),
                                    values.as_mut_ptr(), rows, &mut rows)
        })?;
        timestamps.truncate(rows as usize);
        values.truncate(rows as usize);
        Ok((timestamps, values))
    }

    /// A derived field of two fields per bucket of `date_bin(width, ts, origin)` and group: the count, mean, `m2`, MIN
    /// and MAX of `z = f(x, y)`. `x` and `y` line up row for row under the request's time range; both are rebuilt
    /// values-only into device scratch (8 B per row, never copied to the host). `cells` is row-major
    /// `[n_groups][n_buckets]` (fresh: `DerivedCell::default()`); a cell without pairs stays as it was.
    /// `request.which_mask` must be 0. [`derived_stats`] gives what [`moments_variance`] takes.
    pub fn derived_buckets(
        &self,
        x: &SegmentsView,
        y: &SegmentsView,
        group_of_segment_x: Option<&[u32]>,
        request: &BucketRequest,
        expr: &DerivedExpr,
        cells: &mut [DerivedCell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        check_group_ids(x, group_of_segment_x)?;
        let groups = group_of_segment_x.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_derived_buckets(self.raw(), &x.raw, &y.raw, groups, request, expr, cells.as_mut_ptr()) })
    }

    /// [`Context::derived_buckets`] for several batches per field, merged as one batch per field.
    pub fn derived_buckets_list(
        &self,
        xs: &[SegmentsView],
        ys: &[SegmentsView],
        group_of_segment_x: Option<&[Option<&[u32]>]>,
        request: &BucketRequest,
        expr: &DerivedExpr,
        cells: &mut [DerivedCell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        if let Some(groups) = group_of_segment_x {
            if groups.len() != xs.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), xs.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(xs.len());
        for (k, view) in xs.iter().enumerate() {
            let groups = group_of_segment_x.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let x_inputs: Vec<*const sys::mdb_segments> = xs.iter().map(|view| &view.raw as *const _).collect();
        let y_inputs: Vec<*const sys::mdb_segments> = ys.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_derived_buckets_list(self.raw(), x_inputs.as_ptr(), x_inputs.len() as u32, y_inputs.as_ptr(),
                                          y_inputs.len() as u32, group_pointers.as_ptr(), request, expr,
                                          cells.as_mut_ptr())
        })
    }

    /// The linear trend of a field over time: per bucket of `date_bin(width, ts, origin)` and group one
    /// [`ComomentsCell`] with `x` = the time offset of a point inside its bucket (microseconds, in `[0, width)`) and
    /// `y` = its value - `regr_slope(field, ts)`, `regr_r2`, `corr` and `covar_*` follow with [`comoments_finish`],
    /// whose intercept is the fitted value at the bucket's first instant. The points are those of
    /// [`Context::moments_buckets`]; no point is materialised and no timestamp column is built. `cells` is row-major
    /// `[n_groups][n_buckets]` (fresh: `ComomentsCell::default()`); the batch is merged into it, and a cell without
    /// points stays as it was, so [`comoments_merge`] applies. `request.which_mask` must be 0.
    pub fn trend_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &BucketRequest,
        cells: &mut [ComomentsCell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_trend_buckets(self.raw(), &segments.raw, groups, request, cells.as_mut_ptr()) })
    }

    /// [`Context::trend_buckets`] for several batches at once (rows in the order of the slice), merged as one batch.
    /// `group_of_segment`: `None`, or one entry per batch (`None`: that batch's rows in group 0).
    pub fn trend_buckets_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &BucketRequest,
        cells: &mut [ComomentsCell],
    ) -> Result<()> {
        check_bucket_cells(request, cells.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_trend_buckets_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                        request, cells.as_mut_ptr())
        })
    }

    /// Time-weighted averages and integrals: per bucket `[origin + b * width, origin + (b + 1) * width)` and group
    /// one [`IntegralCell`] - the microseconds on which the series is defined and its integral over them - with the
    /// value between two linked rows interpolated (`MDB_INTEGRAL_LINEAR`) or carried forward (`MDB_INTEGRAL_STEP`).
    /// Rows are linked when they share a group, time moves forward and the gap is within `request.max_gap`; the rule
    /// holds inside a segment and across segments, not across calls: cut batches at series boundaries. `cells` is
    /// row-major `[n_groups][n_buckets]` (fresh: `IntegralCell::default()`); the batch is merged into it, so
    /// [`integral_merge`] and [`integral_average`] apply. `request.buckets` takes no time range and `which_mask` 0.
    pub fn integral_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &IntegralRequest,
        cells: &mut [IntegralCell],
    ) -> Result<()> {
        check_bucket_cells(&request.buckets, cells.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_integral_buckets(self.raw(), &segments.raw, groups, request, cells.as_mut_ptr()) })
    }

    /// [`Context::integral_buckets`] for several batches at once (rows in the order of the slice), merged as one
    /// batch: a linked interval may cross from one batch to the next. `group_of_segment`: `None`, or one entry per
    /// batch (`None`: that batch's rows in group 0).
    pub fn integral_buckets_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &IntegralRequest,
        cells: &mut [IntegralCell],
    ) -> Result<()> {
        check_bucket_cells(&request.buckets, cells.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_integral_buckets_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                           request, cells.as_mut_ptr())
        })
    }

    /// Changes between consecutive rows: per bucket `[origin + b * width, origin + (b + 1) * width)` and group one
    /// [`ChangeCell`] over the linked pairs whose later row lies in the bucket - how many, how many fell, the time
    /// they span, the sums of the rises, of the falls and of the values after a fall, the largest rise and fall.
    /// Rows are linked as for [`Context::integral_buckets`]; a pair is never cut. `cells` is row-major
    /// `[n_groups][n_buckets]` (fresh: `ChangeCell::default()`); the batch is merged into it, so [`change_merge`] and
    /// [`change_finish`] apply. `request.buckets` takes no time range and `which_mask` 0.
    pub fn change_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &ChangeRequest,
        cells: &mut [ChangeCell],
    ) -> Result<()> {
        check_bucket_cells(&request.buckets, cells.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_change_buckets(self.raw(), &segments.raw, groups, request, cells.as_mut_ptr()) })
    }

    /// [`Context::change_buckets`] for several batches at once (rows in the order of the slice), merged as one batch:
    /// a linked pair may cross from one batch to the next. `group_of_segment`: `None`, or one entry per batch
    /// (`None`: that batch's rows in group 0).
    pub fn change_buckets_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &ChangeRequest,
        cells: &mut [ChangeCell],
    ) -> Result<()> {
        check_bucket_cells(&request.buckets, cells.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_change_buckets_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                         request, cells.as_mut_ptr())
        })
    }

    /// The value of a series at the instants `origin + k * width`, `k < n_buckets`: per instant and group one
    /// [`SampleCell`]. A row on an instant contributes its value; between two linked rows the value is interpolated
    /// (`MDB_SAMPLE_LINEAR`) or the earlier one carried forward (`MDB_SAMPLE_STEP`); `MDB_SAMPLE_EXACT` takes rows
    /// only. Rows are linked as for [`Context::integral_buckets`]. `cells` is row-major `[n_groups][n_instants]`
    /// (fresh: `SampleCell::default()`); the batch is merged into it, so [`sample_merge`] and [`sample_values`] apply.
    /// `request.instants` takes no time range and `which_mask` 0.
    pub fn sample_at(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &SampleRequest,
        cells: &mut [SampleCell],
    ) -> Result<()> {
        check_bucket_cells(&request.instants, cells.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe { sys::mdb_sample_at(self.raw(), &segments.raw, groups, request, cells.as_mut_ptr()) })
    }

    /// [`Context::sample_at`] for several batches at once (rows in the order of the slice), sampled as one batch: a
    /// linked interval may cross from one batch to the next. `group_of_segment`: `None`, or one entry per batch
    /// (`None`: that batch's rows in group 0).
    pub fn sample_at_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &SampleRequest,
        cells: &mut [SampleCell],
    ) -> Result<()> {
        check_bucket_cells(&request.instants, cells.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_sample_at_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32, request,
                                    cells.as_mut_ptr())
        })
    }

    /// Episodes: the maximal runs of rows that pass the request's value filter, each row but the first continuing
    /// its predecessor - same group, time not stepping back, at most `request.max_gap` later - ordered by
    /// `first_row`; SQL's gaps-and-islands over the filtered rows, computed on the segments. Rows are numbered as the
    /// masks number them. Returns the episodes of at least `min_count` rows and `min_duration` microseconds, the rows
    /// under the time range and the passing rows among them. Only the episodes cross PCIe.
    pub fn episodes(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &EpisodesRequest,
    ) -> Result<(Vec<Episode>, u64, u64)> {
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        let mut out: *mut sys::mdb_episodes_result = std::ptr::null_mut();
        check(unsafe { sys::mdb_episodes(self.raw(), &segments.raw, groups, request, &mut out) })?;
        Ok(take_episodes(out))
    }

    /// [`Context::episodes`] for several batches at once (rows in the order of the slice), folded as one batch: an
    /// episode may cross from one batch to the next, `first_segment` counts through the list.
    /// `group_of_segment`: `None`, or one entry per batch (`None`: that batch's rows in group 0).
    pub fn episodes_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &EpisodesRequest,
    ) -> Result<(Vec<Episode>, u64, u64)> {
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        let mut out: *mut sys::mdb_episodes_result = std::ptr::null_mut();
        check(unsafe {
            sys::mdb_episodes_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32, request,
                                   &mut out)
        })?;
        Ok(take_episodes(out))
    }

    /// The moments of one field per value cell of another - the power curve: per bucket of
    /// `date_bin(width, ts, origin)`, group and cell of `x` the count, the mean and `m2` of the `y` values of the pairs
    /// whose `x` value falls in the cell (the cell rule of [`hist_cell_of`] under `edges`). The pairs are those of
    /// [`Context::comoments_buckets`]. `cells` is row-major `[n_groups][n_buckets][edges.len() + 1]` (fresh:
    /// `MomentsCell::default()`); the batches are merged into it and a cell without pairs stays as it was, so
    /// [`moments_merge`] and [`moments_variance`] apply. `request.which_mask` must be 0.
    pub fn binned_buckets(
        &self,
        x: &SegmentsView,
        y: &SegmentsView,
        group_of_segment_x: Option<&[u32]>,
        request: &BucketRequest,
        edges: &[f32],
        cells: &mut [MomentsCell],
    ) -> Result<()> {
        check_hist_bucket_cells(request, edges.len() as u64 + 1, cells.len())?;
        check_group_ids(x, group_of_segment_x)?;
        let groups = group_of_segment_x.map_or(std::ptr::null(), |groups| groups.as_ptr());
        let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
        check(unsafe {
            sys::mdb_binned_buckets(self.raw(), &x.raw, &y.raw, groups, request, edges.as_ptr(), n_edges, cells.as_mut_ptr())
        })
    }

    /// [`Context::binned_buckets`] for several batches per field (rows in the order of each slice), merged as one
    /// batch per field: the cuts of `xs` and `ys` need not coincide. `group_of_segment_x`: `None`, or one entry per
    /// batch of `xs` (`None`: that batch's rows in group 0).
    pub fn binned_buckets_list(
        &self,
        xs: &[SegmentsView],
        ys: &[SegmentsView],
        group_of_segment_x: Option<&[Option<&[u32]>]>,
        request: &BucketRequest,
        edges: &[f32],
        cells: &mut [MomentsCell],
    ) -> Result<()> {
        check_hist_bucket_cells(request, edges.len() as u64 + 1, cells.len())?;
        if let Some(groups) = group_of_segment_x {
            if groups.len() != xs.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), xs.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(xs.len());
        for (k, view) in xs.iter().enumerate() {
            let groups = group_of_segment_x.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let x_inputs: Vec<*const sys::mdb_segments> = xs.iter().map(|view| &view.raw as *const _).collect();
        let y_inputs: Vec<*const sys::mdb_segments> = ys.iter().map(|view| &view.raw as *const _).collect();
        let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
        check(unsafe {
            sys::mdb_binned_buckets_list(self.raw(), x_inputs.as_ptr(), x_inputs.len() as u32, y_inputs.as_ptr(),
                                         y_inputs.len() as u32, group_pointers.as_ptr(), request, edges.as_ptr(), n_edges,
                                         cells.as_mut_ptr())
        })
    }

    /// A histogram of the values of `segments` inside `time_range`, without materialising a data point: replaces
    /// GridExec -> AggregateExec for a distribution. `counts` is row-major `[n_groups][edges.len() + 1]` and the
    /// points are ADDED to it; a value falls in the cell numbered by the edges at or below it in totalOrder.
    /// `group_of_segment`: one id per segment row (`None`: all in group 0).
    pub fn hist(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        n_groups: u32,
        edges: &[f32],
        time_range: Option<(i64, i64)>,
        counts: &mut [u64],
    ) -> Result<()> {
        check_hist_cells(n_groups, edges, counts.len())?;
        check_group_ids(segments, group_of_segment)?;
        let request = hist_request(edges, n_groups, time_range);
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        check(unsafe {
            sys::mdb_hist_batch(self.raw(), &segments.raw, groups, &request, edges.as_ptr(), counts.as_mut_ptr())
        })
    }

    /// [`Context::hist`] for several batches at once (rows in the order of the slice), counted as one batch.
    /// `group_of_segment`: `None`, or one entry per batch (`None`: that batch's rows in group 0).
    pub fn hist_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        n_groups: u32,
        edges: &[f32],
        time_range: Option<(i64, i64)>,
        counts: &mut [u64],
    ) -> Result<()> {
        check_hist_cells(n_groups, edges, counts.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let request = hist_request(edges, n_groups, time_range);
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_hist_batch_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                     &request, edges.as_ptr(), counts.as_mut_ptr())
        })
    }

    /// [`Context::hist`] per bucket of `date_bin(width, ts, origin)` and group, in one pass: `counts` is row-major
    /// `[n_groups][n_buckets][edges.len() + 1]` and the points `Context::agg_buckets` counts for the same request are
    /// ADDED to it. `request.which_mask` must be 0.
    pub fn hist_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &BucketRequest,
        edges: &[f32],
        counts: &mut [u64],
    ) -> Result<()> {
        check_hist_bucket_cells(request, edges.len() as u64 + 1, counts.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
        check(unsafe {
            sys::mdb_hist_buckets(self.raw(), &segments.raw, groups, request, edges.as_ptr(), n_edges, counts.as_mut_ptr())
        })
    }

    /// [`Context::hist_buckets`] for several batches at once (rows in the order of the slice), counted as one batch.
    /// `group_of_segment`: `None`, or one entry per batch (`None`: that batch's rows in group 0).
    pub fn hist_buckets_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &BucketRequest,
        edges: &[f32],
        counts: &mut [u64],
    ) -> Result<()> {
        check_hist_bucket_cells(request, edges.len() as u64 + 1, counts.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_hist_buckets_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                       request, edges.as_ptr(), n_edges, counts.as_mut_ptr())
        })
    }

    /// The microseconds one field spent in each value cell, per bucket of `date_bin(width, ts, origin)` and group:
    /// `dwell` is row-major `[n_groups][n_buckets][edges.len() + 1]` and the batch is ADDED to it. Between two linked
    /// rows (the rule of [`Context::integral_buckets`]) the earlier value is held up to the later row; the cells are
    /// those of [`Context::hist_buckets`]. `request.method` must be [`MDB_DWELL_STEP`]; [`dwell_merge`] and
    /// [`dwell_share`] apply.
    pub fn dwell_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &DwellRequest,
        edges: &[f32],
        dwell: &mut [u64],
    ) -> Result<()> {
        check_hist_bucket_cells(&request.buckets, edges.len() as u64 + 1, dwell.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
        check(unsafe {
            sys::mdb_dwell_buckets(self.raw(), &segments.raw, groups, request, edges.as_ptr(), n_edges, dwell.as_mut_ptr())
        })
    }

    /// [`Context::dwell_buckets`] for several batches at once (rows in the order of the slice), folded as one batch: a
    /// link may cross from one batch to the next. `group_of_segment`: `None`, or one entry per batch (`None`: that
    /// batch's rows in group 0).
    pub fn dwell_buckets_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &DwellRequest,
        edges: &[f32],
        dwell: &mut [u64],
    ) -> Result<()> {
        check_hist_bucket_cells(&request.buckets, edges.len() as u64 + 1, dwell.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_dwell_buckets_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                        request, edges.as_ptr(), n_edges, dwell.as_mut_ptr())
        })
    }

    /// The linked pairs of rows of one field by the value cells they go from and to, per bucket of
    /// `date_bin(width, ts, origin)` and group: `counts` is row-major `[n_groups][n_buckets][n_cells][n_cells]` with
    /// `n_cells = edges.len() + 1`, indexed `[from][to]`, and the batch is ADDED to it. Rows are linked by the rule of
    /// [`Context::integral_buckets`]; a pair belongs to the bucket of its later row, as in [`Context::change_buckets`];
    /// the cells are those of [`Context::hist_buckets`]. [`transit_merge`] and [`transit_crossings`] apply.
    pub fn transit_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &TransitRequest,
        edges: &[f32],
        counts: &mut [u64],
    ) -> Result<()> {
        check_transit_counts(&request.buckets, edges.len(), counts.len())?;
        check_group_ids(segments, group_of_segment)?;
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
        check(unsafe {
            sys::mdb_transit_buckets(self.raw(), &segments.raw, groups, request, edges.as_ptr(), n_edges, counts.as_mut_ptr())
        })
    }

    /// [`Context::transit_buckets`] for several batches at once (rows in the order of the slice), folded as one batch:
    /// a pair may cross from one batch to the next. `group_of_segment`: `None`, or one entry per batch (`None`: that
    /// batch's rows in group 0).
    pub fn transit_buckets_list(
        &self,
        segments: &[SegmentsView],
        group_of_segment: Option<&[Option<&[u32]>]>,
        request: &TransitRequest,
        edges: &[f32],
        counts: &mut [u64],
    ) -> Result<()> {
        check_transit_counts(&request.buckets, edges.len(), counts.len())?;
        if let Some(groups) = group_of_segment {
            if groups.len() != segments.len() {
                return Err(HipError(format!("{} group arrays for {} batches", groups.len(), segments.len())));
            }
        }
        let mut group_pointers = Vec::with_capacity(segments.len());
        for (k, view) in segments.iter().enumerate() {
            let groups = group_of_segment.and_then(|groups| groups[k]);
            check_group_ids(view, groups)?;
            group_pointers.push(groups.map_or(std::ptr::null(), |groups| groups.as_ptr()));
        }
        let n_edges = u32::try_from(edges.len()).unwrap_or(u32::MAX);
        let inputs: Vec<*const sys::mdb_segments> = segments.iter().map(|view| &view.raw as *const _).collect();
        check(unsafe {
            sys::mdb_transit_buckets_list(self.raw(), inputs.as_ptr(), group_pointers.as_ptr(), inputs.len() as u32,
                                          request, edges.as_ptr(), n_edges, counts.as_mut_ptr())
        })
    }

    /// [`Context::quantile`] per bucket of `date_bin(width, ts, origin)` and group, in
    /// [`MDB_QUANTILE_BUCKETS_PASSES`] passes whatever the number of cells: row-major `[n_groups][n_buckets]` entries,
    /// each `None` for a cell without a point, else the `(lo, hi)` order statistics of every `q` and the cell's number
    /// of points. At most [`MDB_QUANTILE_BUCKETS_MAX_Q`] quantiles per call; `request.which_mask` must be 0.
    pub fn quantile_buckets(
        &self,
        segments: &SegmentsView,
        group_of_segment: Option<&[u32]>,
        request: &BucketRequest,
        q: &[f64],
    ) -> Result<Vec<Option<(Vec<(f32, f32)>, u64)>>> {
        check_group_ids(segments, group_of_segment)?;
        let cells = (request.n_groups as u64).checked_mul(request.n_buckets)
            .and_then(|cells| usize::try_from(cells).ok())
            .and_then(|cells| cells.checked_mul(q.len().max(1)).map(|_| cells))
            .ok_or_else(|| HipError("n_groups * n_buckets * n_q overflows".to_string()))?;
        let (mut lo, mut hi) = (vec![0f32; cells * q.len()], vec![0f32; cells * q.len()]);
        let mut n_points = vec![0u64; cells];
        let groups = group_of_segment.map_or(std::ptr::null(), |groups| groups.as_ptr());
        let n_q = u32::try_from(q.len()).unwrap_or(u32::MAX);
        check(unsafe {
            sys::mdb_quantile_buckets(self.raw(), &segments.raw, groups, request, q.as_ptr(), n_q, lo.as_mut_ptr(),
                                      hi.as_mut_ptr(), n_points.as_mut_ptr())
        })?;
        Ok((0..cells)
            .map(|cell| {
                if n_points[cell] == 0 {
                    return None;
                }
                let at = cell * q.len();
                Some((lo[at..at + q.len()].iter().copied().zip(hi[at..at + q.len()].iter().copied()).collect(),
                      n_points[cell]))
            })
            .collect())
    }

    /// Exact order statistics of the values of `segments` inside `time_range`, in totalOrder: for every `q` in
    /// [0, 1] the points of rank floor and ceil of `q * (n - 1)`, and `n`, the number of points (`None` when there is
    /// none). What DataFusion's `median` / `percentile_cont` compute from the rebuilt points is
    /// `lo + (hi - lo) * fraction` with [`quantile_positions`]; `approx_percentile_cont` approximates the same. At
    /// most 16 quantiles per call.
    pub fn quantile(
        &self,
        segments: &SegmentsView,
        time_range: Option<(i64, i64)>,
        q: &[f64],
    ) -> Result<Option<(Vec<(f32, f32)>, u64)>> {
        let (t_lo, t_hi) = time_range.unwrap_or((i64::MIN, i64::MAX));
        let (mut lo, mut hi) = (vec![0f32; q.len()], vec![0f32; q.len()]);
        let mut n_points = 0u64;
        let n_q = u32::try_from(q.len()).unwrap_or(u32::MAX);
        check(unsafe {
            sys::mdb_quantile_batch(self.raw(), &segments.raw, t_lo, t_hi, q.as_ptr(), n_q, lo.as_mut_ptr(),
                                    hi.as_mut_ptr(), &mut n_points)
        })?;
        if n_points == 0 {
            return Ok(None);
        }
        Ok(Some((lo.into_iter().zip(hi).collect(), n_points)))
    }

    /// Replaces the body of `try_compress_univariate_time_series` after its two argument checks
    /// (compression.rs:202-211): fits PMC-Mean / Swing / MacaqueV on the GPU and builds the batch
    /// `CompressedSegmentBatchBuilder::finish` builds (types.rs:492-516).
    pub fn compress_univariate(
        &self,
        uncompressed_timestamps: &TimestampArray,
        uncompressed_values: &ValueArray,
        error_bound: ErrorBound,
        compressed_schema: Arc<Schema>,
        tag_values: &[String],
        field_column_index: i16,
    ) -> Result<RecordBatch> {
        // compression.rs:202-206: the library reads `len` timestamps and `len` values.
        if uncompressed_timestamps.len() != uncompressed_values.len() {
            return Err(HipError(
                "Uncompressed timestamps and uncompressed values have different lengths.".to_owned(),
            ));
        }
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::mdb_compress_series(
                self.raw(),
                uncompressed_timestamps.values().as_ptr(),
                uncompressed_values.values().as_ptr(),
                uncompressed_values.len() as u64,
                error_bound.into(),
                &mut raw,
            )
        })?;
        let owned = Arc::new(OwnedSegments(NonNull::new(raw).expect("success with a null result")));
        let rows = unsafe { owned.0.as_ref() }.seg.n as usize;
        record_batch_of_rows(&owned.whole_columns()?, 0, rows, compressed_schema, tag_values, field_column_index)
    }

    /// Compresses MANY univariate time series with one launch per distinct error bound and returns one
    /// batch of segments per chunk, in the order of `chunks`. This is the form the fitter is fast in: a
    /// launch fits one chunk per lane, so 10^4 chunks take about as long as one. The chunks are read where
    /// they lie (slices of the caller's arrays); chunks that share a timestamp array - the fields of one
    /// series - have it looked at once.
    pub fn compress_chunks(&self, chunks: &[SeriesChunk]) -> Result<Vec<RecordBatch>> {
        let mut compressed: Vec<Option<RecordBatch>> = vec![None; chunks.len()];
        let mut done = vec![false; chunks.len()];
        for first in 0..chunks.len() {
            if done[first] {
                continue;
            }
            // Every chunk with this error bound (an error bound is an argument of the launch).
            let bound: sys::mdb_error_bound = chunks[first].error_bound.into();
            let mut group = Vec::new();
            let mut list = Vec::new();
            for index in first..chunks.len() {
                let chunk = &chunks[index];
                let chunk_bound: sys::mdb_error_bound = chunk.error_bound.into();
                if done[index] || chunk_bound != bound {
                    continue;
                }
                if chunk.timestamps.len() != chunk.values.len() {
                    return Err(HipError(
                        "Uncompressed timestamps and uncompressed values have different lengths.".to_owned(),
                    ));
                }
                done[index] = true;
                group.push(index);
                list.push(sys::mdb_chunk {
                    ts: chunk.timestamps.as_ptr(),
                    values: chunk.values.as_ptr(),
                    n: chunk.values.len() as u64,
                });
            }
            let mut raw = ptr::null_mut();
            check(unsafe { sys::mdb_compress_chunk_list(self.raw(), list.as_ptr(), list.len() as u64, bound, &mut raw) })?;
            let owned = Arc::new(OwnedSegments(NonNull::new(raw).expect("success with a null result")));
            // Segments come back grouped by chunk, in chunk order.
            let (rows, chunk_index) = unsafe {
                let c = owned.0.as_ref();
                if c.seg.n > 0 && c.chunk_index.is_null() {
                    return Err(HipError("The library returned segments without their chunk index.".to_owned()));
                }
                (c.seg.n as usize, std::slice::from_raw_parts(c.chunk_index, c.seg.n as usize))
            };
            let whole = owned.whole_columns()?; // (validated once; every chunk's batch is a slice of it)
            let mut row = 0;
            for (position, &index) in group.iter().enumerate() {
                let begin = row;
                while row < rows && chunk_index[row] as usize == position {
                    row += 1;
                }
                let chunk = &chunks[index];
                compressed[index] = Some(record_batch_of_rows(
                    &whole,
                    begin,
                    row - begin,
                    chunk.compressed_schema.clone(),
                    chunk.tag_values,
                    chunk.field_column_index,
                )?);
            }
        }
        Ok(compressed.into_iter().map(|batch| batch.expect("every chunk is in one group")).collect())
    }

    /// `try_split_and_compress_univariate_time_series` (compression.rs:147-179): the field columns of ONE
    /// time series, which share its timestamps; `fields` = (values, error bound, field column index).
    pub fn split_and_compress(
        &self,
        uncompressed_timestamps: &TimestampArray,
        fields: &[(&ValueArray, ErrorBound, i16)],
        compressed_schema: Arc<Schema>,
        tag_values: &[String],
    ) -> Result<Vec<RecordBatch>> {
        let chunks: Vec<SeriesChunk> = fields
            .iter()
            .map(|(values, error_bound, field_column_index)| SeriesChunk {
                timestamps: uncompressed_timestamps.values(),
                values: values.values(),
                error_bound: *error_bound,
                compressed_schema: compressed_schema.clone(),
                tag_values,
                field_column_index: *field_column_index,
            })
            .collect();
        self.compress_chunks(&chunks)
    }
}

/// One univariate time series to compress: its sorted data points where they lie, and what the resulting
/// batch of segments is labelled with (`CompressedSegmentBatchBuilder::new`, types.rs:444-470).
pub struct SeriesChunk<'a> {
    pub timestamps: &'a [i64],
    pub values: &'a [f32],
    pub error_bound: ErrorBound,
    pub compressed_schema: Arc<Schema>,
    pub tag_values: &'a [String],
    pub field_column_index: i16,
}

/// Number of columns of `QUERY_COMPRESSED_SCHEMA` (crates/modelardb_types/src/schemas.rs:40-52); the tag
/// columns of a batch of segments follow them.
const QUERY_COMPRESSED_COLUMNS: usize = 9;

/// An outstanding [`Context::grid_submit`]: the library reconstructs the batches on one of its worker
/// threads while the caller goes on (polls its input for the next batches, hands out slices of the
/// previous result). Keeps the input batches alive, since the library reads their Arrow buffers until
/// [`GridTicket::wait`] returns. Dropping a ticket waits for the job and frees what it made.
pub struct GridTicket {
    raw: Option<NonNull<sys::mdb_grid_ticket>>,
    batches: Vec<RecordBatch>,
    n_tag_columns: usize,
}

// The ticket is only a handle; the library synchronises the job behind it.
unsafe impl Send for GridTicket {}

impl Drop for GridTicket {
    fn drop(&mut self) {
        if let Some(raw) = self.raw.take() {
            unsafe { sys::mdb_grid_cancel(raw.as_ptr()) };
        }
    }
}

/// What [`GridTicket::wait`] returns: the columns of the new current batch of a `GridStream`.
pub struct PipelinedGridOutput {
    /// Leftovers first, then the reconstructed data points (grid_exec.rs:302-320).
    pub timestamps: TimestampArray,
    pub values: ValueArray,
    /// One array per tag column: every segment's tag once per data point reconstructed from it
    /// (grid_exec.rs:339-346), the leftovers' tags in front. The strings are not copied: long ones stay in
    /// the data buffers of the input batches, which the arrays share.
    pub tags: Vec<StringViewArray>,
    pub metrics: GridMetrics,
    /// Segments and data points of this submit (a stream sizes its next submit by them).
    pub segments: u64,
    pub rows_created: u64,
}

impl Context {
    /// Starts the reconstruction of ALL segments of `batches` (each with the columns of
    /// `QUERY_COMPRESSED_SCHEMA` followed by the table's tag columns) as one launch and returns at once.
    /// `reserve_front`: room in front of the result for the rows the stream has left (`batch_size` is
    /// enough: a stream only asks for more when it has fewer than that). Replaces, together with
    /// [`GridTicket::wait`], grid_exec.rs:261-364 for several input batches at once.
    pub fn grid_submit(
        &self,
        batches: Vec<RecordBatch>,
        reserve_front: usize,
        time_range: Option<(i64, i64)>,
    ) -> Result<GridTicket> {
        assert!(!batches.is_empty(), "grid_submit needs at least one batch.");
        let n_tag_columns = batches[0].num_columns() - QUERY_COMPRESSED_COLUMNS;
        let views: Vec<SegmentsView> = batches.iter().map(SegmentsView::from_record_batch).collect();
        // Per batch: the views of its tag arrays, and where its data buffers start in the output tag
        // column's list of buffers (buffer 0 is the ticket's own, for long leftover strings).
        let mut tag_views: Vec<Vec<*const sys::mdb_view16>> = Vec::with_capacity(batches.len());
        let mut tag_shifts: Vec<Vec<i32>> = Vec::with_capacity(batches.len());
        let mut next_buffer = vec![1i32; n_tag_columns];
        for batch in &batches {
            assert_eq!(batch.num_columns(), QUERY_COMPRESSED_COLUMNS + n_tag_columns);
            let mut views_of_batch = Vec::with_capacity(n_tag_columns);
            let mut shifts_of_batch = Vec::with_capacity(n_tag_columns);
            for tag_column in 0..n_tag_columns {
                let tags = tag_array(batch, tag_column);
                views_of_batch.push(tags.views().as_ptr().cast::<sys::mdb_view16>());
                shifts_of_batch.push(next_buffer[tag_column]);
                next_buffer[tag_column] += tags.data_buffers().len() as i32;
            }
            tag_views.push(views_of_batch);
            tag_shifts.push(shifts_of_batch);
        }
        let inputs: Vec<sys::mdb_grid_input> = (0..batches.len())
            .map(|index| sys::mdb_grid_input {
                segments: views[index].raw,
                tag_views: if n_tag_columns > 0 { tag_views[index].as_ptr() } else { ptr::null() },
                tag_buffer_shift: if n_tag_columns > 0 { tag_shifts[index].as_ptr() } else { ptr::null() },
            })
            .collect();
        let (flags, t_lo, t_hi) = match time_range {
            Some((lo, hi)) => (sys::MDB_GRID_HAS_RANGE, lo, hi),
            None => (0, 0, 0),
        };
        let request = sys::mdb_grid_request {
            flags,
            n_tag_columns: n_tag_columns as u32,
            t_lo,
            t_hi,
            reserve_front: reserve_front as u64,
        };
        let mut raw = ptr::null_mut();
        // The structs and the small tables above are copied by the library before this returns; the
        // Arrow buffers behind them are kept alive by `batches` in the ticket.
        check(unsafe {
            sys::mdb_grid_submit(self.raw(), inputs.as_ptr(), inputs.len() as u32, &request, &mut raw)
        })?;
        drop(views);
        Ok(GridTicket {
            raw: Some(NonNull::new(raw).expect("success with a null ticket")),
            batches,
            n_tag_columns,
        })
    }
}

fn tag_array(batch: &RecordBatch, tag_column: usize) -> &StringViewArray {
    batch
        .column(QUERY_COMPRESSED_COLUMNS + tag_column)
        .as_any()
        .downcast_ref::<StringViewArray>()
        .expect("The tag columns of a batch of segments should be StringViewArrays.")
}

impl GridTicket {
    /// Segment rows this ticket was made from.
    pub fn segments(&self) -> usize {
        self.batches.iter().map(RecordBatch::num_rows).sum()
    }

    /// Blocks until the batches are reconstructed and returns the columns of the stream's new current
    /// batch: `leftover_*` (the rows of the current batch that have not been handed out, fewer than the
    /// `reserve_front` of the submit) in front, the new data points behind them. The arrays wrap memory of
    /// the library (page-locked for the data points) without copying; the last of them to be dropped
    /// returns it to the library's pools.
    pub fn wait(
        mut self,
        leftover_timestamps: &[i64],
        leftover_values: &[f32],
        leftover_tags: &[StringViewArray],
    ) -> Result<PipelinedGridOutput> {
        assert_eq!(leftover_timestamps.len(), leftover_values.len());
        assert_eq!(leftover_tags.len(), self.n_tag_columns);
        let leftovers = leftover_timestamps.len();
        let ticket = self.raw.take().expect("a ticket is waited for once");
        let mut raw = ptr::null_mut();
        check(unsafe { sys::mdb_grid_wait(ticket.as_ptr(), &mut raw) })?;
        let block = Arc::new(GridBlock(NonNull::new(raw).expect("success with a null result")));
        let result = unsafe { block.0.as_ref() };
        assert!(leftovers as u64 <= result.reserved_front, "more leftovers than room was reserved for");
        let total = leftovers + result.n as usize;
        let (timestamps, values) = unsafe {
            let first_timestamp = result.timestamps.sub(leftovers);
            let first_value = result.values.sub(leftovers);
            ptr::copy_nonoverlapping(leftover_timestamps.as_ptr(), first_timestamp, leftovers);
            ptr::copy_nonoverlapping(leftover_values.as_ptr(), first_value, leftovers);
            (
                Buffer::from_custom_allocation(
                    NonNull::new_unchecked(first_timestamp.cast::<u8>()),
                    8 * total,
                    block.clone(),
                ),
                Buffer::from_custom_allocation(NonNull::new_unchecked(first_value.cast::<u8>()), 4 * total, block.clone()),
            )
        };
        let mut tags = Vec::with_capacity(self.n_tag_columns);
        for (tag_column, leftover) in leftover_tags.iter().enumerate() {
            assert_eq!(leftover.len(), leftovers);
            // The leftovers' views in front of the replicated ones. Their long strings are copied into a
            // buffer of the new array (buffer 0), so that old inputs can be dropped.
            let mut leftover_payload: Vec<u8> = Vec::new();
            let first_view = unsafe {
                let replicated = sys::mdb_grid_result_tag_views(result, tag_column as u32);
                assert!(!replicated.is_null(), "the result has fewer tag columns than the submit asked for");
                let first_view = replicated.sub(leftovers);
                for row in 0..leftovers {
                    let value = leftover.value(row).as_bytes();
                    let mut view = sys::mdb_view16 { length: value.len() as i32, u: [0; 12] };
                    if value.len() <= 12 {
                        view.u[..value.len()].copy_from_slice(value);
                    } else {
                        view.u[..4].copy_from_slice(&value[..4]);
                        view.u[4..8].copy_from_slice(&0i32.to_le_bytes());
                        view.u[8..12].copy_from_slice(&(leftover_payload.len() as i32).to_le_bytes());
                        leftover_payload.extend_from_slice(value);
                    }
                    first_view.add(row).write(view);
                }
                first_view
            };
            let views = unsafe {
                Buffer::from_custom_allocation(NonNull::new_unchecked(first_view.cast::<u8>()), 16 * total, block.clone())
            };
            // The same order `grid_submit` numbered them in (`tag_buffer_shift`).
            let mut buffers = vec![Buffer::from_vec(leftover_payload)];
            for batch in &self.batches {
                buffers.extend(tag_array(batch, tag_column).data_buffers().iter().cloned());
            }
            // Every view is a copy of a view of a valid StringViewArray with its buffer index moved to where
            // that buffer is in `buffers`, or was written above from a &str: valid by construction, and
            // validating 16 bytes per data point again would cost more than reconstructing the point.
            tags.push(unsafe { StringViewArray::new_unchecked(ScalarBuffer::new(views, 0, total), buffers, None) });
        }
        Ok(PipelinedGridOutput {
            timestamps: TimestampArray::new(ScalarBuffer::new(timestamps, 0, total), None),
            values: ValueArray::new(ScalarBuffer::new(values, 0, total), None),
            tags,
            metrics: result.metrics,
            segments: result.n_segments,
            rows_created: result.n,
        })
    }
}

/// A row-selection bitmap in device memory (include/mdb.h, "row masks"): row `r` is bit `r % 64` of word `r / 64`,
/// the bits at and beyond `n_rows` are zero - byte for byte an Arrow boolean bitmap. Made by [`Context::row_mask`],
/// filled and consumed by the `mdb_*_dev` calls on batches that are resident on the device (through
/// [`RowMask::as_ptr`] / [`RowMask::as_mut_ptr`]); freed on drop.
pub struct RowMask<'a> {
    context: &'a Context,
    words: *mut u64,
    n_rows: u64,
    cap_words: u64,
}

impl RowMask<'_> {
    pub fn n_rows(&self) -> u64 {
        self.n_rows
    }

    pub fn cap_words(&self) -> u64 {
        self.cap_words
    }

    pub fn as_ptr(&self) -> *const u64 {
        self.words
    }

    pub fn as_mut_ptr(&mut self) -> *mut u64 {
        self.words
    }

    /// `self = self op other` (`MDB_MASK_AND` / `OR` / `XOR` / `ANDNOT`), or `self = !self` (`MDB_MASK_NOT`, `other`
    /// None); returns the number of set bits.
    pub fn combine(&mut self, op: u32, other: Option<&RowMask>) -> Result<u64> {
        if let Some(other) = other {
            if other.n_rows != self.n_rows {
                return Err(HipError(format!("masks over {} and {} rows", self.n_rows, other.n_rows)));
            }
        }
        let mut n_set = 0u64;
        check(unsafe {
            sys::mdb_mask_combine_dev(self.context.raw(), op, self.words, other.map_or(ptr::null(), |mask| mask.words),
                                      self.words, self.n_rows, &mut n_set)
        })?;
        Ok(n_set)
    }

    /// The mask on the host, as the `BooleanBuffer` a `BooleanArray` is made of (no bit is touched on the way).
    pub fn download(&self) -> Result<BooleanBuffer> {
        let mut words = vec![0u64; self.n_rows.div_ceil(64) as usize];
        check(unsafe {
            sys::mdb_dev_download(self.context.raw(), words.as_mut_ptr().cast(), self.words.cast_const().cast(),
                                  8 * words.len() as u64)
        })?;
        Ok(BooleanBuffer::new(Buffer::from_vec(words), 0, self.n_rows as usize))
    }
}

impl Drop for RowMask<'_> {
    fn drop(&mut self) {
        unsafe { sys::mdb_dev_free(self.context.raw(), self.words.cast()) };
    }
}

/// Segments returned by the compressor (host memory), freed when the last array made from them is dropped.
struct OwnedSegments(NonNull<sys::mdb_segments_owned>);

unsafe impl Send for OwnedSegments {}
unsafe impl Sync for OwnedSegments {}
impl std::panic::RefUnwindSafe for OwnedSegments {}

impl Drop for OwnedSegments {
    fn drop(&mut self) {
        unsafe { sys::mdb_segments_free(self.0.as_ptr()) };
    }
}

impl OwnedSegments {
    /// The nine segment columns over ALL rows of the result, wrapping the library's memory (kept alive by
    /// `self`). Built - and the three BinaryView columns validated - ONCE per result: a result of one launch
    /// is cut into a batch per chunk, and validating every view of the joint result for every chunk would
    /// cost (chunks x segments) view checks where (segments) suffice.
    fn whole_columns(self: &Arc<Self>) -> Result<Vec<ArrayRef>> {
        let owned = unsafe { self.0.as_ref() };
        let segments = &owned.seg;
        let n = segments.n as usize;
        if n > 0 && owned.error.is_null() {
            return Err(HipError("The library returned segments without their error column.".to_owned()));
        }
        let wrap = |pointer: *const u8, bytes: usize| -> Buffer {
            match NonNull::new(pointer.cast_mut()) {
                Some(pointer) if bytes > 0 => unsafe { Buffer::from_custom_allocation(pointer, bytes, self.clone()) },
                _ => Buffer::from(Vec::<u8>::new()),
            }
        };
        let binary_view = |column: &sys::mdb_binview_col| -> Result<ArrayRef> {
            if column.n_buffers < 0 || (column.n_buffers > 0 && (column.buffers.is_null() || column.buffer_sizes.is_null())) {
                return Err(HipError("The library returned a malformed BinaryView column.".to_owned()));
            }
            let mut buffers = Vec::with_capacity(column.n_buffers as usize);
            for index in 0..column.n_buffers as usize {
                let (pointer, size) = unsafe { (*column.buffers.add(index), *column.buffer_sizes.add(index)) };
                buffers.push(wrap(pointer, size as usize));
            }
            // A ScalarBuffer<u128> must be 16-byte aligned. The library's views are (every column of a result
            // begins on a 16-byte boundary of an allocation of the C++ runtime or at a multiple of 64 bytes in
            // one); a pointer that is not is copied instead of trusted.
            let view_bytes = if (column.views as usize) % std::mem::align_of::<u128>() == 0 {
                wrap(column.views.cast(), 16 * n)
            } else {
                let copied: Vec<u128> = (0..n)
                    .map(|row| unsafe { ptr::read_unaligned(column.views.cast::<u128>().add(row)) })
                    .collect();
                Buffer::from_vec(copied)
            };
            let views = ScalarBuffer::<u128>::new(view_bytes, 0, n);
            // try_new checks every view against `buffers` (length, buffer index, offset, prefix).
            let array = BinaryViewArray::try_new(views, buffers, None).map_err(|error| HipError(error.to_string()))?;
            Ok(Arc::new(array))
        };
        Ok(vec![
            Arc::new(Int8Array::new(ScalarBuffer::new(wrap(segments.model_type_id.cast(), n), 0, n), None)) as ArrayRef,
            Arc::new(TimestampArray::new(ScalarBuffer::new(wrap(segments.start_time.cast(), 8 * n), 0, n), None)) as ArrayRef,
            Arc::new(TimestampArray::new(ScalarBuffer::new(wrap(segments.end_time.cast(), 8 * n), 0, n), None)) as ArrayRef,
            binary_view(&segments.timestamps)?,
            Arc::new(ValueArray::new(ScalarBuffer::new(wrap(segments.min_value.cast(), 4 * n), 0, n), None)) as ArrayRef,
            Arc::new(ValueArray::new(ScalarBuffer::new(wrap(segments.max_value.cast(), 4 * n), 0, n), None)) as ArrayRef,
            binary_view(&segments.values)?,
            binary_view(&segments.residuals)?,
            Arc::new(Float32Array::new(ScalarBuffer::new(wrap(owned.error.cast(), 4 * n), 0, n), None)) as ArrayRef,
        ])
    }
}

/// Rows `[first, first + length)` of `whole` (see [`OwnedSegments::whole_columns`]) as a batch with
/// `compressed_schema` (`CompressedSegmentBatchBuilder::finish`, types.rs:492-516): slices of the arrays over
/// the whole result, so cutting one result into a batch per chunk copies and checks nothing.
fn record_batch_of_rows(
    whole: &[ArrayRef],
    first: usize,
    length: usize,
    compressed_schema: Arc<Schema>,
    tag_values: &[String],
    field_column_index: i16,
) -> Result<RecordBatch> {
    assert!(whole.iter().all(|column| first + length <= column.len()));
    let mut columns: Vec<ArrayRef> = Vec::with_capacity(compressed_schema.fields().len());
    columns.extend(whole.iter().map(|column| column.slice(first, length)));
    columns.push(Arc::new(iter::repeat_n(field_column_index, length).collect::<Int16Array>()));
    for tag_value in tag_values {
        columns.push(Arc::new(iter::repeat_n(Some(tag_value), length).collect::<StringViewArray>()));
    }
    RecordBatch::try_new(compressed_schema, columns).map_err(|error| HipError(error.to_string()))
}

/// A process-wide context for call sites that have no natural owner for one (the accumulators are
/// created per partition by a closure, `try_compress_univariate_time_series` is a free function).
/// Device from `MODELARDB_HIP_DEVICE` (default 0). Calls through it are serialised; a `GridStream`
/// takes a context of its own from [`pooled_context`] instead.
pub fn shared_context() -> &'static Context {
    static SHARED: std::sync::LazyLock<Context> = std::sync::LazyLock::new(|| {
        let device = default_device();
        Context::new(device).unwrap_or_else(|error| panic!("libmdb_hip cannot use device {device}: {error}"))
    });
    &SHARED
}

/// A context of its own for an operator that lives as long as a query (`GridStream`), taken from a pool the
/// process keeps: a fresh context costs a stream and, with its first batches, device scratch (≈ 15 ms added to
/// the first query), a pooled one nothing. Goes back to the pool when dropped.
pub fn pooled_context() -> Result<PooledContext> {
    let recycled = CONTEXT_POOL.lock().unwrap_or_else(|poisoned| poisoned.into_inner()).pop();
    let context = match recycled {
        Some(context) => context,
        None => Context::new(default_device())?,
    };
    Ok(PooledContext(Some(context)))
}

static CONTEXT_POOL: std::sync::Mutex<Vec<Context>> = std::sync::Mutex::new(Vec::new());

/// At most this many idle contexts are kept; each keeps what `mdb_set_scratch_limit` allows it.
const CONTEXT_POOL_CAPACITY: usize = 64;
/// Device scratch an idle pooled context may keep (256 MiB: the scratch of an 8 192-segment batch is ≈ 100 MB).
const POOLED_SCRATCH_LIMIT: u64 = 256 << 20;

pub struct PooledContext(Option<Context>);

impl std::ops::Deref for PooledContext {
    type Target = Context;
    fn deref(&self) -> &Context {
        self.0.as_ref().expect("the context is only taken out when the guard is dropped")
    }
}

impl Drop for PooledContext {
    fn drop(&mut self) {
        if let Some(context) = self.0.take() {
            let _ = context.set_scratch_limit(POOLED_SCRATCH_LIMIT);
            let mut pool = CONTEXT_POOL.lock().unwrap_or_else(|poisoned| poisoned.into_inner());
            if pool.len() < CONTEXT_POOL_CAPACITY {
                pool.push(context);
            }
        }
    }
}

/// The HIP device this process computes on: `MODELARDB_HIP_DEVICE`, default 0 (one process per GPU).
pub fn default_device() -> i32 {
    std::env::var("MODELARDB_HIP_DEVICE").ok().and_then(|text| text.parse().ok()).unwrap_or(0)
}
