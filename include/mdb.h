/*
 * mdb.h - C ABI of libmdb_hip.so: ModelarDB's model-compression / grid / segment-aggregate hot
 * path as hand-written HIP kernels for gfx950 (MI355X).
 *
 * This is the drop-in boundary. The reference has no plugin API: modelardb_storage and
 * modelardb_server call the modelardb_compression crate directly. Each entry point below replaces
 * one of those call sites at BATCH granularity (one call per Arrow RecordBatch instead of one per
 * row); INTEGRATION.md shows the Rust `extern "C"` block and the patched call sites.
 *
 * Conventions (mirroring the reference's own C API, crates/modelardb_embedded/src/capi.rs:58-80
 * and bindings/c/modelardb_embedded.h:74-78,202-203):
 *   - every function returns 0 on success and 1 on failure;
 *   - mdb_last_error() returns the message of the last failure on the calling thread, valid until
 *     the next failing call on that thread;
 *   - malformed segments (the reference panics: models/mod.rs:170,237, macaque_v.rs:224,279-280,
 *     types.rs:316-318,391,405) are error returns, never aborts;
 *   - inputs are borrowed for the duration of the call; outputs are written into caller-allocated
 *     buffers, or returned as mdb_segments_owned that the caller frees with mdb_segments_free().
 *   - a context (mdb_ctx) owns one HIP stream and scratch memory. Calls on one context are
 *     serialised by an internal mutex; use one context per thread for concurrency.
 *
 * "host" entry points take host pointers (straight into Arrow buffers) and return after the
 * results are in host memory. "_dev" entry points take device pointers, enqueue on the context's
 * stream and return after the stream has been synchronised unless stated otherwise.
 *
 * Paths in the citations are relative to the reference repository root.
 */
#ifndef MDB_H
#define MDB_H

#include "mdb_format.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdb_ctx mdb_ctx;

/* ---- lifetime ------------------------------------------------------------------------------- */

/* Create a context on HIP device `device`. Constructor convention of capi.rs:218-229. */
int mdb_init(int device, mdb_ctx **ctx);
int mdb_close(mdb_ctx *ctx);
/* Another context on the device of `ctx` (its own stream and scratch memory): what an operator that
 * wants two batches in flight - the copy of one overlapping the kernels of the next - asks for.
 * (All contexts of a device share one pool of page-locked result blocks, so a context made per query does
 * not pay for pinning memory again; and a clone that is closed is kept - up to four of them - for the next
 * mdb_clone of the same context, stream and scratch included, until that context is closed itself.) */
int mdb_clone(mdb_ctx *ctx, mdb_ctx **out);
const char *mdb_last_error(void);
/* "libmdb_hip <version> gfx950"; never fails. */
const char *mdb_version(void);
/* Use an externally created hipStream_t (e.g. torch's current stream) instead of the context's. */
int mdb_set_stream(mdb_ctx *ctx, void *hip_stream);
/* Give back the working memory the context has grown for the batches seen so far (device scratch,
 * page-locked staging and the recycled result blocks); the next call grows what it needs again.
 * A context keeps this memory between calls because allocating is slow - a fit of 10^10 points
 * leaves tens of GB behind - so a long-lived owner calls this after an unusually large batch.
 * released_bytes (may be NULL): device bytes given back. Results and segments already handed out
 * stay valid. */
int mdb_trim(mdb_ctx *ctx, uint64_t *released_bytes);
/* The same, automatically: after every call on this context, device scratch beyond `bytes` is given back
 * (largest allocations first; 0, the default, keeps everything). For owners of many contexts - one
 * GridStream per field column - each of which would otherwise keep what its largest batch needed. A clone
 * (mdb_clone) starts with the limit of the context it was made from.
 * No call is refused for the limit, with one exception: mdb_comoments_buckets* fails when its y column alone
 * (4 B per row under the time range) is larger than a limit other than 0, even where other operators take more
 * transient scratch for the same batch. The caller then cuts the batch by series or lifts the limit for the call. */
int mdb_set_scratch_limit(mdb_ctx *ctx, uint64_t bytes);
/* Name, CU count, HBM bytes of the context's device. */
int mdb_device_info(mdb_ctx *ctx, char *name, uint64_t name_cap, int32_t *compute_units,
                    uint64_t *hbm_bytes);

/* ---- device memory owned by the library (so the bench needs no other allocator) -------------- */

int mdb_dev_alloc(mdb_ctx *ctx, uint64_t bytes, void **dev_ptr);
int mdb_dev_free(mdb_ctx *ctx, void *dev_ptr);
int mdb_dev_upload(mdb_ctx *ctx, void *dev_dst, const void *host_src, uint64_t bytes);
int mdb_dev_download(mdb_ctx *ctx, void *host_dst, const void *dev_src, uint64_t bytes);
int mdb_dev_sync(mdb_ctx *ctx);
/* Copy a host batch of segments (Arrow buffers) to the device; the result has on_device = 1. */
int mdb_segments_upload(mdb_ctx *ctx, const mdb_segments *host, mdb_segments_owned **dev);
/* Copy a device batch back; the result has on_device = 0 and one data buffer per column (several if the
 * column's payloads exceed 2 GiB). */
int mdb_segments_download(mdb_ctx *ctx, const mdb_segments_owned *dev, mdb_segments_owned **host);
void mdb_segments_free(mdb_segments_owned *segments);
/* mdb_segments_upload checks every out-of-line view of a HOST batch against the column's data buffers
 * (a view that points outside them is an error, never a wild device read). A batch that is ALREADY on
 * the device and was not made by this library (mdb_segments_upload / mdb_compress_chunks*) must be
 * well formed: the "_dev" entry points follow buffer_index and offset without looking. This runs the
 * same check on such a batch (views in device memory, buffer_sizes a host array as everywhere). */
int mdb_segments_validate_dev(mdb_ctx *ctx, const mdb_segments *dev);

/* ---- grid: replaces the per-row loop of GridStream::grid_and_append_to_leftovers_in_current_batch
 *      (crates/modelardb_storage/src/query/grid_exec.rs:323-356) which calls
 *      modelardb_compression::grid (crates/modelardb_compression/src/models/mod.rs:190-251) ------ */

/* Number of data points the batch reconstructs to (sum over rows of the timestamps a row
 * decompresses to), so the caller can allocate the outputs. */
int mdb_grid_count(mdb_ctx *ctx, const mdb_segments *in, uint64_t *n_out);

/* Reconstruct every data point of every segment, in segment order. out_ts/out_val need `cap`
 * elements (cap >= mdb_grid_count). out_rows_per_segment (optional, n entries) is what the caller
 * uses to replicate tag values (grid_exec.rs:339-346). metrics is optional (grid_exec.rs:511-518). */
int mdb_grid_batch(mdb_ctx *ctx, const mdb_segments *in, int64_t *out_ts, float *out_val,
                   uint32_t *out_rows_per_segment, uint64_t cap, uint64_t *n_out,
                   mdb_grid_metrics *metrics);

/* Device resident variant: `in` holds device pointers (e.g. from mdb_segments_upload or
 * mdb_compress_chunks_dev), outputs are device buffers. out_ts may be NULL: then only the values
 * are reconstructed, which is what a join of several field columns of the same series needs for
 * every field after the first (SortedJoinExec zips per-field GridExec outputs that share their
 * timestamps, crates/modelardb_storage/src/query/sorted_join_exec.rs:252-310). */
int mdb_grid_count_dev(mdb_ctx *ctx, const mdb_segments *in, uint64_t *n_out);
int mdb_grid_batch_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t *out_ts, float *out_val,
                       uint32_t *out_rows_per_segment, uint64_t cap, uint64_t *n_out,
                       mdb_grid_metrics *metrics);

/* Predicate pushdown: only the data points with t_lo <= timestamp <= t_hi are
 * reconstructed. The reference's GridStream reconstructs every point of every segment the Parquet
 * filter let through and prunes afterwards (grid_exec.rs:366-387); the result is the same rows in
 * the same order. rows_per_segment and the row counters of `metrics` count the rows produced. */
int mdb_grid_count_range(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi,
                         uint64_t *n_out);
int mdb_grid_batch_range(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi,
                         int64_t *out_ts, float *out_val, uint32_t *out_rows_per_segment, uint64_t cap,
                         uint64_t *n_out, mdb_grid_metrics *metrics);
int mdb_grid_count_range_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi,
                             uint64_t *n_out);
int mdb_grid_batch_range_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi,
                             int64_t *out_ts, float *out_val, uint32_t *out_rows_per_segment,
                             uint64_t cap, uint64_t *n_out, mdb_grid_metrics *metrics);

/* One-call form for host callers: sizes, reconstructs and copies back in one go (one upload of the
 * segments, one prepass, one copy from the device) into page-locked memory owned by the library,
 * which the caller wraps without copying and returns with mdb_grid_result_free() (allowed after
 * mdb_close()). flags: MDB_GRID_HAS_RANGE applies the predicate t_lo <= timestamp <= t_hi;
 * MDB_GRID_VALUES_ONLY skips the timestamps (result->timestamps is NULL): the second and later
 * field columns of a SortedJoinExec only contribute their values (sorted_join_exec.rs:268-275), so
 * their timestamps need not cross PCIe. Two to three times
 * faster end to end than mdb_grid_count + mdb_grid_batch into pageable memory.
 * reserve_front asks for that many writable rows in front of the reconstructed points, so a
 * GridStream can put the leftovers of its previous batch there (grid_exec.rs:302-320) and hand
 * out slices of the block without copying the new points at all. */
#define MDB_GRID_HAS_RANGE 1u
#define MDB_GRID_VALUES_ONLY 2u
int mdb_grid_batch_owned(mdb_ctx *ctx, const mdb_segments *in, uint32_t flags, int64_t t_lo,
                         int64_t t_hi, uint64_t reserve_front, mdb_grid_result **out);
void mdb_grid_result_free(mdb_grid_result *result);

/* The library's switches (the MDB_* names of INTEGRATION.md 2.6: A/B timings and the scheduling modes the tests force;
 * the defaults are what a deployment runs). The process's environment is read ONCE, by the first call that asks for a
 * switch: no getenv() inside a call. mdb_set_option sets one switch for the whole process without touching the
 * environment (value NULL: back to "not set"); mdb_reload_options reads the environment again (what a test that has
 * changed it calls). No counterpart in the reference (its settings are
 * crates/modelardb_server/src/configuration.rs, none of which reaches this path). */
int mdb_set_option(const char *name, const char *value);
int mdb_reload_options(void);
/* What a switch is set to (NULL: not set). The text stays valid for the life of the process (setting the switch again
 * or reloading the table makes later look-ups return another text and leaves this one as it is), so mdb_set_option and
 * mdb_reload_options may be called while other threads are inside calls: a call sees a switch as it was when it asked.
 * The price of that: every DISTINCT value a switch has ever had is kept (a few bytes each, never freed) - switches are
 * for deployments and tests, not a per-query channel; a caller that sets one to ever-changing values grows the table. */
const char *mdb_option(const char *name);

/* Pipelined form, for an operator that is polled (GridStream::poll_next, grid_exec.rs:402-429): submit
 * returns at once with a ticket, a worker thread of the library reconstructs the batch on the context or
 * on a clone of it that the library keeps (submits alternate between the two), so the kernels of one
 * batch run while the previous batch's points still cross PCIe; mdb_grid_wait blocks until the result
 * is in host memory. Two submits may be outstanding per context before the third one queues behind them.
 *   - inputs: one OR SEVERAL RecordBatches of segments, reconstructed by one launch as if they were one
 *     batch (rows in the order of the list): the batches DataSourceExec hands a GridStream hold 8 192
 *     segments, and a launch pays off from 10^5 (SURVEY 8(f) N2 - the caller keeps polling its input and
 *     submits what it has got, no concat_batches on the host). rows_per_segment and n_segments of the
 *     result run over all inputs.
 *   - tags (grid_exec.rs:339-346): with request->n_tag_columns > 0 every input carries the views of its
 *     tag arrays; the result then also holds, per tag column, the views repeated once per reconstructed
 *     row (mdb_grid_result_tag_views), written by the library's host threads past the cache while the
 *     next batch is on the GPU. The strings themselves are not copied: an output view points into the
 *     input's data buffers, which the caller lists behind its own (tag_buffer_shift).
 *   - the mdb_grid_input / mdb_grid_request structs and the small tables they point at are copied by
 *     submit; the Arrow buffers behind them must stay alive until mdb_grid_wait / mdb_grid_cancel returns.
 *   - mdb_grid_wait consumes the ticket whether it succeeds or not; a stream that is dropped with a ticket
 *     outstanding calls mdb_grid_cancel (waits for the job and frees its result).
 * Replaces, together with mdb_grid_result_*: grid_exec.rs:261-391 for several input batches at once. */
typedef struct mdb_grid_ticket mdb_grid_ticket;
int mdb_grid_submit(mdb_ctx *ctx, const mdb_grid_input *inputs, uint32_t n_inputs,
                    const mdb_grid_request *request, mdb_grid_ticket **ticket);
int mdb_grid_wait(mdb_grid_ticket *ticket, mdb_grid_result **out);
void mdb_grid_cancel(mdb_grid_ticket *ticket);
/* The replicated views of tag column `column` of a result of mdb_grid_submit: result->n views, the view of
 * the first reconstructed row first, with result->reserved_front writable views in front of it (the
 * leftovers' tags). NULL if the request had fewer tag columns. Freed with the result. */
mdb_view16 *mdb_grid_result_tag_views(const mdb_grid_result *result, uint32_t column);
/* The replication by itself, for callers that keep their own output buffers (host arithmetic, no
 * context): out[k] = views[i] for the rows_per_segment[i] rows of segment i, buffer_index of views longer
 * than 12 bytes moved by buffer_shift. out needs sum(rows_per_segment) views (checked against out_cap).
 * Large fills are split over the library's host threads and written with streaming stores. */
int mdb_replicate_views(const mdb_view16 *views, const uint32_t *rows_per_segment, uint64_t n_segments,
                        int32_t buffer_shift, mdb_view16 *out, uint64_t out_cap);

/* ---- aggregates: replaces Model{Count,Min,Max,Sum,Avg}Accumulator::update_batch
 *      (crates/modelardb_storage/src/optimizer/model_simple_aggregates.rs:345-358, 395-401,
 *      438-444, 481-513, 553-587) which call modelardb_compression::{len,sum}
 *      (crates/modelardb_compression/src/models/mod.rs:98-184) ---------------------------------- */

/* Fold the batch into *inout for the aggregates in which_mask (MDB_AGG_*). COUNT/MIN/MAX are exact;
 * SUM adds the f32 per-segment sums in f64 with a fixed (deterministic) tree order, so it can
 * differ from the reference's sequential f64 accumulation in the last bits (the reference's own
 * tests allow 0.001 %: crates/modelardb_server/tests/integration_test.rs:1155-1171). */
int mdb_agg_batch(mdb_ctx *ctx, const mdb_segments *in, uint32_t which_mask, mdb_agg_state *inout);
int mdb_agg_batch_dev(mdb_ctx *ctx, const mdb_segments *in, uint32_t which_mask,
                      mdb_agg_state *inout);
/* The same for SEVERAL RecordBatches of segments (rows in the order of the list), uploaded and folded as one
 * batch: an accumulator is handed 8 192 segments per update_batch (model_simple_aggregates.rs:345, 481, 553) and
 * nobody sees its state before state() (:367, 523, 590), while a call costs the same for 8 192 and for 262 144
 * segments (the batches are gathered by the caller, without copying, and passed here). */
int mdb_agg_batch_list(mdb_ctx *ctx, const mdb_segments *const *inputs, uint32_t n_inputs, uint32_t which_mask,
                       mdb_agg_state *inout);

/* Extension (BASELINE config 3): aggregates over the data points with
 * t_lo <= timestamp <= t_hi without materialising them. The reference has no such operator: any
 * WHERE on the timestamp falls back to GridExec + filter + AggregateExec
 * (model_simple_aggregates.rs:284-302), and that result is the parity oracle: COUNT / MIN / MAX of the
 * reconstructed points inside the range, SUM their f64 sum. */
int mdb_agg_batch_range(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi,
                        uint32_t which_mask, mdb_agg_state *inout);
int mdb_agg_batch_range_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi,
                            uint32_t which_mask, mdb_agg_state *inout);
/* The list form (mdb_agg_batch_list under a time range): what the accumulators of a ranged query fold their
 * gathered batches with. The patched optimizer rule (rust/patches/0002) accepts AggregateExec <- FilterExec(a
 * conjunction of comparisons of the timestamp column with literals) <- SortedJoinExec <- GridExec <-
 * DataSourceExec(the start_time / end_time filter TimeSeriesTable::scan derived from the same comparisons,
 * query/time_series_table.rs:290-373) and hands [t_lo, t_hi] to the accumulators it creates. */
int mdb_agg_batch_range_list(mdb_ctx *ctx, const mdb_segments *const *inputs, uint32_t n_inputs, int64_t t_lo,
                             int64_t t_hi, uint32_t which_mask, mdb_agg_state *inout);

/* Extension: the aggregates per time bucket and group - what the reference computes for
 * SELECT <tags>, date_bin(width, ts, origin), COUNT/MIN/MAX/SUM/AVG(field) ... GROUP BY 1, 2 with GridExec, the
 * date_bin / range filter and AggregateExec (its model-based rule only takes an empty GROUP BY,
 * model_simple_aggregates.rs:219), computed on the segments without materialising a point.
 *   inout: row-major [n_groups][n_buckets] states. Each cell is folded with the rules of mdb_agg_merge, for the
 *     aggregates in request->which_mask as mdb_agg_batch folds them; a cell with no points is left exactly as it
 *     was (a fresh cell stays {0, 0, FLT_MAX, -FLT_MAX}).
 *   group_of_segment: one group id per segment row (the caller derives it from the tag columns: one id per series
 *     or per tag combination); NULL puts every segment in group 0. The list form takes one such array per input
 *     (NULL, or a NULL entry: group 0).
 *   Parity: the reference's fallback plan (GridExec -> date_bin / range filter -> GROUP BY). COUNT, MIN and MAX are
 *     exact; SUM is the f64 sum of a cell's f32 points, within the 0.001 % of the other aggregates.
 *   Determinism: for the same input, request and form (host, dev or list), results are bit-identical from run to
 *     run, and the three forms agree bit for bit; no float atomics. MDB_AGG_BUCKET_SLICE_PAIRS
 *     changes the order in which a cell's partials are added, within the tolerance.
 *   Errors (mdb_last_error set, inout untouched): width <= 0, n_groups == 0, n_groups * n_buckets overflowing,
 *     a group id >= n_groups (every row is checked), a malformed segment among those the request reaches (the error
 *     classes of mdb_agg_batch). As for mdb_agg_batch_range, a segment outside every bucket or outside
 *     [t_lo, t_hi] is not examined: the reference's scan prunes such segments on start_time / end_time too.
 *   n_buckets == 0 (or an empty batch) does nothing and succeeds. Bucket arithmetic does not overflow for any
 *     origin, width, t_lo or t_hi. */
int mdb_agg_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                    const mdb_bucket_request *request, mdb_agg_state *inout);
/* All device pointers: the segments, group_of_segment and inout are in HBM. */
int mdb_agg_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                        const mdb_bucket_request *request, mdb_agg_state *inout);
/* Several host batches (rows in the order of the list) folded as one batch, as mdb_agg_batch_list does. */
int mdb_agg_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs,
                         const uint32_t *const *group_of_segment, uint32_t n_inputs,
                         const mdb_bucket_request *request, mdb_agg_state *inout);

/* Extension: a value predicate pushed down to the segments - WHERE field op literal [AND ts op literal ...], see
 * mdb_value_filter (mdb_format.h). The reference rewrites only predicates on the timestamp column
 * (query/time_series_table.rs:290-370); one on the field stays in a FilterExec above GridExec, which rebuilds every
 * point first (query/grid_exec.rs:366-387), and an aggregate under it misses the model-based rule, whose input must
 * be a SortedJoinExec (optimizer/model_simple_aggregates.rs:214-243).
 *   Grid: replaces GridExec -> FilterExec. The rows are exactly those of mdb_grid_batch_range(t_lo, t_hi) without
 *     the ones whose value fails, in segment order and point order within a segment. out_rows_per_segment (may be
 *     NULL) counts the rows of each segment (0: none). The row counters of metrics count the rows produced, the
 *     segment counters are mdb_grid_batch_range's for the same t_lo / t_hi.
 *   Aggregates: replace GridExec -> FilterExec -> AggregateExec. The passing points are folded into *inout with the
 *     rules of mdb_agg_batch_range: COUNT / MIN / MAX exact, SUM the f64 sum of the passing f32 points within the
 *     0.001 % of the other aggregates; no passing point leaves *inout as mdb_agg_batch_range leaves it. The host,
 *     dev and list forms agree bit for bit, and so do two runs (a fixed reduction tree, no float atomics).
 *   An empty value interval (v_lo above v_hi in totalOrder, [c, c)) is valid and selects nothing.
 *   Errors (mdb_last_error set, outputs untouched): unknown flag bits, reserved != 0, cap too small, and the error
 *     classes of the range calls. */
int mdb_grid_count_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, uint64_t *n_out);
int mdb_grid_batch_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, int64_t *out_ts,
                              float *out_val, uint32_t *out_rows_per_segment, uint64_t cap, uint64_t *n_out,
                              mdb_grid_metrics *metrics);
/* One-call form for host callers, as mdb_grid_batch_owned (one upload, the work on the device, one copy back into
 * page-locked memory, the same reserve_front): only the passing rows and rows_per_segment cross PCIe. Freed by
 * mdb_grid_result_free. */
int mdb_grid_batch_filter_owned(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter,
                                uint64_t reserve_front, mdb_grid_result **out);
int mdb_agg_batch_filter(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, uint32_t which_mask,
                         mdb_agg_state *inout);
/* The segments in HBM (inout stays a host pointer, as for mdb_agg_batch_range_dev). */
int mdb_agg_batch_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter,
                             uint32_t which_mask, mdb_agg_state *inout);
/* Several host batches (rows in the order of the list) folded as one batch, as mdb_agg_batch_list does. */
int mdb_agg_batch_filter_list(mdb_ctx *ctx, const mdb_segments *const *inputs, uint32_t n_inputs,
                              const mdb_value_filter *filter, uint32_t which_mask, mdb_agg_state *inout);

/* Extension: mdb_agg_buckets* with a value predicate - SELECT <tags>, date_bin(...), AGG(field) ... WHERE field op
 * literal [AND ts op literal ...] GROUP BY 1, 2, which the reference answers with GridExec -> FilterExec ->
 * AggregateExec. A point (t, v) of segment row i counts in cell (group_of_segment[i], floor((t - origin) / width))
 * when that bucket is in [0, n_buckets), t lies in both [request->t_lo, request->t_hi] and [filter->t_lo,
 * filter->t_hi], and v passes the filter's value bounds in totalOrder (as for mdb_agg_batch_filter).
 *   The result is mdb_agg_buckets of the same batch with every other point removed: the same fold rules, the same
 *     pairs, entries and reduction tree; a cell without a passing point is left exactly as it was. COUNT, MIN and
 *     MAX are exact, SUM within 0.001 %. A filter with MDB_VALUE_NO_LO | MDB_VALUE_NO_HI over the whole time range
 *     gives the cells of mdb_agg_buckets bit for bit on a batch of finite values.
 *   Determinism: as mdb_agg_buckets (the three forms and two runs agree bit for bit; no float atomics).
 *   Errors (mdb_last_error set, inout untouched): a NULL argument; unknown filter flag bits or reserved != 0 (checked
 *     before the device is used); every error of mdb_agg_buckets for the same request with its time range narrowed
 *     to the intersection - a predicate never hides a bad group id or a malformed segment. An empty value interval
 *     or an empty intersection of the time ranges is valid: it selects nothing, the group ids are still checked. */
int mdb_agg_buckets_filter(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                           const mdb_bucket_request *request, const mdb_value_filter *filter, mdb_agg_state *inout);
/* All device pointers but request and filter: the segments, group_of_segment and inout are in HBM. */
int mdb_agg_buckets_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                               const mdb_bucket_request *request, const mdb_value_filter *filter,
                               mdb_agg_state *inout);
/* Several host batches (rows in the order of the list) folded as one batch, as mdb_agg_buckets_list does. */
int mdb_agg_buckets_filter_list(mdb_ctx *ctx, const mdb_segments *const *inputs,
                                const uint32_t *const *group_of_segment, uint32_t n_inputs,
                                const mdb_bucket_request *request, const mdb_value_filter *filter,
                                mdb_agg_state *inout);

/* Extension: row masks - a predicate on one field column selects the rows of another:
 *   SELECT AVG(active_power) FROM turbine WHERE wind_speed > 12.0 AND rotor_speed <= 14.5 AND ts BETWEEN ...
 * which the reference answers with GridExec per field -> SortedJoinExec -> FilterExec (-> AggregateExec): every point of
 * every named field is rebuilt, zipped by row position (query/sorted_join_exec.rs:278-310) and a BooleanArray per
 * predicate decides the rows. Here that bitmap is made from one field's segments and consumed by another's without a
 * point of either being materialised.
 *   The mask: over n_rows rows, ceil(n_rows / 64) uint64_t words in device memory; row r is bit r % 64 of word r / 64
 *     (on a little-endian host byte for byte an Arrow boolean bitmap, bit r % 8 of byte r / 8: a downloaded mask wraps
 *     as a BooleanBuffer as it is). Bits at and beyond n_rows in the last word are zero after every call that writes a
 *     mask. The rows are those of mdb_grid_batch_range(in, t_lo, t_hi), in that order.
 *   Row alignment: two field batches line up when they hold the same series in the same order with the same
 *     timestamps; row r of one is then the same data point's row in the other, however differently the two were cut
 *     into segments, under any common time range. The consuming calls check the row COUNT only, as the reference does -
 *     but where SortedJoinExec truncates to its shortest input (sorted_join_exec.rs:252-273, a workaround for
 *     half-transferred folders) these calls fail, before writing anything, with a message that names both counts.
 *   Errors (mdb_last_error set, outputs untouched): as stated per call, and the error classes of the range calls. */
#define MDB_MASK_AND 0u
#define MDB_MASK_OR 1u
#define MDB_MASK_XOR 2u
#define MDB_MASK_ANDNOT 3u /* a & ~b */
#define MDB_MASK_NOT 4u    /* ~a; b must be NULL */
/* The mask of `filter` over the rows of mdb_grid_batch_range_dev(in, filter->t_lo, filter->t_hi): a bit is set iff the
 * row's value passes the value bounds in totalOrder (exactly the rows mdb_grid_batch_filter_dev keeps). *n_rows: the
 * number of rows; *n_set (may be NULL): the set bits. Every word the mask owns is written (the buffer need not be
 * cleared). Errors: cap_words below ceil(n_rows / 64), unknown filter flags or reserved != 0. */
int mdb_mask_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, uint64_t *mask,
                        uint64_t cap_words, uint64_t *n_rows, uint64_t *n_set);
/* out = a op b (MDB_MASK_*) over n_rows rows; out may be a or b. The padding bits stay zero (NOT clears the tail).
 * *n_set (may be NULL): the set bits of out. Errors: an unknown op, b != NULL with MDB_MASK_NOT, a NULL mask. */
int mdb_mask_combine_dev(mdb_ctx *ctx, uint32_t op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n_rows,
                         uint64_t *n_set);
/* The rows of mdb_grid_batch_range_dev(in, t_lo, t_hi) whose bit is set, in order. out_ts may be NULL (values only: the
 * second and later fields of a join). out_rows_per_segment and metrics as for mdb_grid_batch_filter_dev (the row
 * counters count the rows produced, the segment counters are the range call's). The number of rows produced is the
 * mask's n_set. Errors: the batch does not have exactly n_rows rows under [t_lo, t_hi]; cap too small. */
int mdb_grid_batch_mask_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const uint64_t *mask,
                            uint64_t n_rows, int64_t *out_ts, float *out_val, uint32_t *out_rows_per_segment, uint64_t cap,
                            uint64_t *n_out, mdb_grid_metrics *metrics);
/* The selected points folded into *inout (a host pointer, as for mdb_agg_batch_range_dev) with the rules of
 * mdb_agg_batch_filter: COUNT / MIN / MAX exact, SUM the f64 sum of the selected f32 points within the 0.001 % of the
 * other aggregates; no selected point leaves *inout as mdb_agg_batch_range leaves it. A fixed reduction tree, no float
 * atomics: two runs agree bit for bit. Errors: the batch does not have exactly n_rows rows under [t_lo, t_hi]. */
int mdb_agg_batch_mask_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const uint64_t *mask,
                           uint64_t n_rows, uint32_t which_mask, mdb_agg_state *inout);
/* One-call forms for host callers: pred_fields[k] is a host batch and filters[k] its predicate; the predicates are
 * ANDed. The time range of the call is the INTERSECTION of all filters' [t_lo, t_hi], applied to every predicate field
 * and to `target` so that the rows line up (an empty intersection selects nothing). target may be one of the predicate
 * batches (the same pointer): it is then uploaded once. Every batch is uploaded once, the masks live in the context's
 * scratch, only the result crosses PCIe. n_preds == 0: mdb_agg_batch_range over the whole time axis / every row.
 * The results agree bit for bit with the _dev calls above on the same batches.
 * Errors: a predicate field whose row count under the range differs from the target's; those of the _dev calls. */
int mdb_agg_batch_where(mdb_ctx *ctx, const mdb_segments *const *pred_fields, const mdb_value_filter *filters,
                        uint32_t n_preds, const mdb_segments *target, uint32_t which_mask, mdb_agg_state *inout);
/* The same for rows, into a page-locked mdb_grid_result as mdb_grid_batch_filter_owned (reserve_front, freed by
 * mdb_grid_result_free). flags: MDB_GRID_VALUES_ONLY (result->timestamps is NULL) or 0; anything else is an error. */
int mdb_grid_batch_where_owned(mdb_ctx *ctx, const mdb_segments *const *pred_fields, const mdb_value_filter *filters,
                               uint32_t n_preds, const mdb_segments *target, uint32_t flags, uint64_t reserve_front,
                               mdb_grid_result **out);

/* Extension: value histograms and exact quantiles -
 *   SELECT approx_percentile_cont(field, 0.95) ... / SELECT median(field) ... WHERE ts BETWEEN ... / a histogram of a
 *   field per series,
 * which the reference answers with GridExec -> AggregateExec (approx_percentile_cont / median are not among the
 * aggregates its model-based rule rewrites, optimizer/model_simple_aggregates.rs: every point is rebuilt first). Here
 * the points are counted per cell on the segments: a PMC-Mean segment is one addition, a Swing segment on regular
 * timestamps one binary search over its point index per edge it crosses, a bit stream is decoded once.
 *   Cells: mdb_hist_request (mdb_format.h): n_cells = n_edges + 1, a point of value v in cell c = the number of edges
 *     e with key(e) <= key(v) in the totalOrder of mdb_value_filter (-0.0 lies below an edge at +0.0, a NaN lands
 *     where its key puts it).
 *   counts: uint64_t [n_groups][n_cells], row-major. A call ADDS the batch's points - exactly the rows of
 *     mdb_grid_batch_range(in, t_lo, t_hi), segment row i in group group_of_segment[i] (NULL: every segment in group 0) -
 *     to them; a fresh histogram is all zeros, a cell that receives nothing is left as it was. Per group the cells'
 *     increments add up to the COUNT of mdb_agg_buckets with one bucket over [t_lo, t_hi]; the increments of cells
 *     a + 1 .. b to the COUNT of mdb_agg_batch_filter with [edges[a], edges[b]).
 *   Determinism: integers only (integer atomics on zeroed scratch cells, folded into counts once the pass has
 *     finished): the three forms and any two runs agree bit for bit.
 *   Errors (mdb_last_error set, counts untouched): a NULL argument; flags or reserved != 0, n_edges outside
 *     1 .. MDB_HIST_MAX_EDGES, edges not strictly increasing in totalOrder (equal keys, descending, -0.0 after +0.0),
 *     n_groups == 0 (all checked before the device is used); n_groups * n_cells counters that do not fit the device; a
 *     group id >= n_groups on ANY row, also one outside the time range; the malformed-segment classes of
 *     mdb_agg_batch_range. An empty batch or an empty time range succeeds and changes nothing. */
int mdb_hist_batch(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                   const mdb_hist_request *request, const float *edges, uint64_t *counts);
/* The segments, group_of_segment and counts are in HBM; request and edges are host pointers. */
int mdb_hist_batch_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                       const mdb_hist_request *request, const float *edges, uint64_t *counts);
/* Several host batches (rows in the order of the list) counted as one batch; group_of_segment[k] (or NULL) per batch. */
int mdb_hist_batch_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                        uint32_t n_inputs, const mdb_hist_request *request, const float *edges, uint64_t *counts);
/* Order statistics of the points inside [t_lo, t_hi] of the whole batch, in totalOrder, exact (what DataFusion's
 * median / percentile_cont compute from the rebuilt points; approx_percentile_cont approximates the same).
 * For q[i] in [0, 1]: p = q[i] * (double)(N - 1), out_lo[i] = the floor(p)-th smallest point (0-based), out_hi[i] =
 * the ceil(p)-th; *n_points = N. N == 0: succeeds, *n_points = 0, out_lo / out_hi untouched. 1 <= n_q <= 16.
 * The batch is uploaded once; the ranks are pinned by repeated histogram passes over the resident copy (edges even in
 * key space, then inside the cell that holds the rank: 12 + 12 + 8 bits, three passes for ranks that share their
 * cells). Interpolation (lo + (hi - lo) * fraction, mdb_quantile_positions) is the caller's.
 * Errors (outputs untouched): a NULL argument, q outside [0, 1] or NaN, n_q out of range, a malformed segment. */
int mdb_quantile_batch(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const double *q, uint32_t n_q,
                       float *out_lo, float *out_hi, uint64_t *n_points);
/* The segments are in HBM. */
int mdb_quantile_batch_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const double *q,
                           uint32_t n_q, float *out_lo, float *out_hi, uint64_t *n_points);
/* Host arithmetic, no context, no GPU: the cell rule (validates the edges as mdb_hist_batch does) ... */
int mdb_hist_cell_of(const float *edges, uint32_t n_edges, float value, uint32_t *cell);
/* ... and the ranks of a quantile: p = q * (double)(n_points - 1), *rank_lo = floor(p), *rank_hi = ceil(p),
 * *fraction = p - floor(p). Errors: n_points == 0, q outside [0, 1] or NaN, a NULL output. */
int mdb_quantile_positions(double q, uint64_t n_points, uint64_t *rank_lo, uint64_t *rank_hi, double *fraction);

/* Extension: M4 downsampling - per bucket of date_bin(width, ts, origin) and group the first, last, lowest and highest
 * data point WITH their timestamps: what a plotting front end asks a time-series store for per pixel column. The
 * reference answers it with GridExec -> AggregateExec(first_value / last_value(field ORDER BY ts), min, max) GROUP BY
 * the date_bin, and a join of the result back onto the points for the timestamps of the minimum and maximum: every
 * point is rebuilt first. Here the cells are computed on the segments and no point is materialised.
 *   request: mdb_bucket_request, unchanged; which_mask must be 0. inout: row-major [n_groups][n_buckets] cells
 *     (mdb_m4_cell, mdb_format.h); a fresh cell is all-zero bytes. group_of_segment as for mdb_agg_buckets.
 *   Which points: exactly those mdb_agg_buckets counts for the same request - bucket floor((t - origin) / width) in
 *     [0, n_buckets) and t in [t_lo, t_hi]; a point of segment row i goes to group group_of_segment[i].
 *   Which of them, with key(v) the totalOrder key of mdb_value_filter:
 *     first = the point with the smallest (t, key(v)), compared lexicographically; last = the largest (t, key(v));
 *     min = the smallest (key(v), t); max = the largest key(v) and, among those, the smallest t; count = how many.
 *     In a group that holds one series timestamps are unique: first / last are first_value / last_value(field ORDER
 *     BY ts), min / max the extreme values at their earliest occurrence.
 *   Each rule is commutative and associative, so a cell depends only on the SET of its points: not on the order of
 *     the segments, on how a batch is cut into calls or list entries, on the slice size
 *     (MDB_AGG_BUCKET_SLICE_PAIRS), on whether the keys had to be sorted, or on the shape of the reduction tree. The
 *     host, dev and list forms agree bit for bit, and so do two runs; folding the halves of a batch into the same
 *     cells, in either order, gives the bytes of the whole batch.
 *   Merging: a call merges its batch into inout by the same rules (mdb_m4_merge_n is that rule on the host, cell by
 *     cell: into[j] = into[j] + from[j]). A cell that receives no point keeps every byte it had.
 *   Against mdb_agg_buckets: count equals its COUNT, always. In a cell without a NaN, v_min / v_max compare equal
 *     (==) to its MIN / MAX. They differ with NaNs: that operator skips them (min_num / max_num), totalOrder places
 *     them (-NaN below -inf, +NaN above +inf), so a cell with a NaN reports it as v_min or v_max. -0.0 is below +0.0.
 *   Errors (mdb_last_error set, inout untouched): a NULL argument, which_mask != 0, and those of mdb_agg_buckets -
 *     width <= 0, n_groups == 0, n_groups * n_buckets overflowing, a group id >= n_groups on any row, a malformed
 *     segment among those the request reaches. An empty batch or n_buckets == 0 succeeds and changes nothing. */
int mdb_m4_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                   const mdb_bucket_request *request, mdb_m4_cell *inout);
/* All device pointers: the segments, group_of_segment and inout are in HBM. */
int mdb_m4_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                       const mdb_bucket_request *request, mdb_m4_cell *inout);
/* Several host batches (rows in the order of the list) folded as one batch, as mdb_agg_buckets_list does. */
int mdb_m4_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                        uint32_t n_inputs, const mdb_bucket_request *request, mdb_m4_cell *inout);
/* Host arithmetic, no context, no GPU: into[j] merged with from[j] for j < n. */
int mdb_m4_merge_n(mdb_m4_cell *into, const mdb_m4_cell *from, uint64_t n);

/* Extension: variance and standard deviation - per bucket of date_bin(width, ts, origin) and group the count, the mean
 * and m2 = the sum of (v - mean)^2: the state of DataFusion's variance accumulators, from which stddev, stddev_pop,
 * var_samp and var_pop follow. The reference answers them with GridExec -> AggregateExec like a median: its
 * model-based rule rewrites only count / min / max / sum / avg
 * (crates/modelardb_storage/src/optimizer/model_simple_aggregates.rs:319-323), so every point is rebuilt first. Here
 * the cells are computed on the segments and no point is materialised.
 *   request: mdb_bucket_request, unchanged; which_mask must be 0. inout: row-major [n_groups][n_buckets] cells
 *     (mdb_moments_cell, mdb_format.h); a fresh cell is all-zero bytes. group_of_segment as for mdb_agg_buckets.
 *   Which points: exactly those mdb_agg_buckets counts for the same request, so count equals its COUNT, always.
 *   How: a run of points (those of one segment in one bucket) is accumulated with sums shifted by the run's first
 *     value K: d = (double)v - (double)K, s1 += d, s2 += d * d; mean = K + s1 / n, m2 = s2 - s1 * s1 / n (0 where
 *     that rounds below 0). A sum of v * v next to the sum of v is not used: at a level of 1e6 with a deviation of 0.5
 *     it loses four digits to cancellation. PMC-Mean on regular timestamps is (n, value, 0) in O(1); Swing is
 *     evaluated point by point, because the rebuilt points are f32 roundings of the line and that rounding is part of
 *     their variance.
 *   Merge rule, the same in mdb_moments_merge_n and in every kernel: with n = na + nb and d = mean_b - mean_a,
 *     mean = mean_a + d * (nb / n), m2 = m2_a + m2_b + d * d * (na * nb / n); an empty side gives the other side's
 *     bytes. A call merges its batch into inout; a cell that receives no point keeps every byte it had. Cells of
 *     equal values have m2 == 0.0 and mean == the value exactly, in any order of merges.
 *   Non-finite points: in a cell that holds a NaN or an infinity count is exact and neither mean nor m2 is finite;
 *     nothing more is promised.
 *   Determinism, as for mdb_agg_buckets' SUM: for the same input, request and form two runs agree bit for bit, and so
 *     do the host, dev and list forms; no float atomics, no atomics on cells. What changes the order of the merges -
 *     MDB_AGG_BUCKET_SLICE_PAIRS, the order of the segments, cutting a batch into calls, whether the keys had to be
 *     sorted - moves mean and m2 by rounding only (the tests allow 2^-44 of the largest |v| and 1e-5 of m2).
 *   Errors (mdb_last_error set, inout untouched): those of mdb_m4_buckets - a NULL argument, which_mask != 0,
 *     width <= 0, n_groups == 0, n_groups * n_buckets overflowing, a group id >= n_groups on any row, a malformed
 *     segment among those the request reaches. An empty batch or n_buckets == 0 succeeds and changes nothing. */
int mdb_moments_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                        const mdb_bucket_request *request, mdb_moments_cell *inout);
/* All device pointers: the segments, group_of_segment and inout are in HBM. */
int mdb_moments_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                            const mdb_bucket_request *request, mdb_moments_cell *inout);
/* Several host batches (rows in the order of the list) folded as one batch, as mdb_agg_buckets_list does. */
int mdb_moments_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                             uint32_t n_inputs, const mdb_bucket_request *request, mdb_moments_cell *inout);
/* Host arithmetic, no context, no GPU: into[j] merged with from[j] by the merge rule, for j < n. */
int mdb_moments_merge_n(mdb_moments_cell *into, const mdb_moments_cell *from, uint64_t n);
/* Host arithmetic, no context, no GPU: variance_out[j] = m2 / (count - ddof) of cells[j]. ddof 0: var_pop (NaN for a
 * count of 0); ddof 1: var_samp (NaN for a count of 1 or less); any other ddof is an error. stddev is its sqrt. */
int mdb_moments_variance(const mdb_moments_cell *cells, uint64_t n, uint32_t ddof, double *variance_out);

/* Extension: covariance and correlation of two fields - per bucket of date_bin(width, ts, origin) and group the count,
 * both means, both m2 and c_xy = the sum of (x - mean_x) * (y - mean_y) over the pairs of the bucket:
 *   SELECT date_bin(...), corr(active_power, wind_speed), regr_slope(active_power, wind_speed) ... GROUP BY 1, turbine
 * corr, covar_samp, covar_pop, regr_slope, regr_intercept and regr_r2 follow from a cell (mdb_comoments_finish). The
 * reference answers them with GridExec per field -> SortedJoinExec -> AggregateExec: its model-based rule rewrites only
 * count / min / max / sum / avg (crates/modelardb_storage/src/optimizer/model_simple_aggregates.rs:319-323), so every
 * point of both fields is rebuilt and zipped by row position (query/sorted_join_exec.rs:278-310). Here x is walked on
 * its segments and nothing of it is materialised; y is rebuilt values-only into a scratch column of 4 B per row that
 * lives in HBM only and never crosses PCIe - the one thing the operator materialises.
 *   x, y: two field columns of the same series with the same timestamps, each cut into segments in its own way (the
 *     alignment rule of the row masks). x is the independent variable: the kinds below are SQL's regr_*(y, x).
 *   request: mdb_bucket_request, unchanged; which_mask must be 0. inout: row-major [n_groups][n_buckets] cells
 *     (mdb_comoments_cell, mdb_format.h); a fresh cell is all-zero bytes. group_of_segment_x: per segment of x, as for
 *     mdb_agg_buckets.
 *   Which points: the rows of mdb_grid_batch_range(x, t_lo, t_hi) and of mdb_grid_batch_range(y, t_lo, t_hi), in
 *     order; row r of one is paired with row r of the other. A pair belongs to the bucket of its x-side timestamp and
 *     the group of its x-side segment, and is counted exactly where mdb_agg_buckets counts the x point for the same
 *     request: count equals that COUNT, always. Rows outside buckets 0 .. n_buckets-1 keep their place in the row
 *     numbering and are not counted.
 *   Alignment: only the row COUNT under [t_lo, t_hi] is checked; a mismatch fails before anything is written, with a
 *     message that names both counts. The cuts of the lists xs and ys need not coincide.
 *   How: a run of pairs (those of one x segment in one bucket) is accumulated around its first pair (Kx, Ky):
 *     dx = (double)x - Kx, dy = (double)y - Ky, sx += dx, sy += dy, sxx += dx * dx, syy += dy * dy, sxy += dx * dy;
 *     means and m2 as for mdb_moments_buckets, c_xy = sxy - sx * sy / n (not clamped).
 *   Merge rule, the same in mdb_comoments_merge_n and in every kernel: means and m2 as mdb_moments_merge_n, and with
 *     dx = mean_xb - mean_xa, dy likewise: c_xy = c_a + c_b + dx * dy * (na * nb / n); an empty side gives the other
 *     side's bytes. A cell that receives no pair keeps every byte it had. A cell in which either field is constant has
 *     c_xy == 0.0 exactly, in any order of merges; a pair of identical fields has m2_x, m2_y and c_xy of the same bytes.
 *   Non-finite points: in a cell that holds a NaN or an infinity in a field count is exact, and that field's mean and
 *     m2 and c_xy are not finite; nothing more is promised.
 *   Determinism, as for mdb_moments_buckets: for the same input, request and form two runs agree bit for bit, and so
 *     do the host, dev and list forms; no float atomics, no atomics on cells. MDB_AGG_BUCKET_SLICE_PAIRS, the order of
 *     the segments and cutting a batch into calls move the f64 members by rounding only.
 *   Scratch: the y column takes 4 B per row under [t_lo, t_hi]. Under mdb_set_scratch_limit a column larger than the
 *     limit is refused with a message that states the bytes needed: cut the batch by series, the cells merge.
 *   Errors (mdb_last_error set, inout untouched): those of mdb_moments_buckets*, a NULL y, the row-count mismatch, the
 *     y column refused, a malformed segment in x or y. An empty batch or n_buckets == 0 succeeds and changes nothing. */
#define MDB_COMOMENTS_COVAR_POP 0u      /* c / n;                        NaN when n = 0 */
#define MDB_COMOMENTS_COVAR_SAMP 1u     /* c / (n - 1);                  NaN when n <= 1 */
#define MDB_COMOMENTS_CORR 2u           /* c / sqrt(m2_x * m2_y);        NaN when n <= 1 or either m2 is 0 */
#define MDB_COMOMENTS_REGR_SLOPE 3u     /* c / m2_x;                     NaN when n <= 1 or m2_x is 0 */
#define MDB_COMOMENTS_REGR_INTERCEPT 4u /* mean_y - slope * mean_x;      as REGR_SLOPE */
#define MDB_COMOMENTS_REGR_R2 5u        /* c * c / (m2_x * m2_y);        as CORR */
int mdb_comoments_buckets(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const uint32_t *group_of_segment_x,
                          const mdb_bucket_request *request, mdb_comoments_cell *inout);
/* All device pointers: both batches, group_of_segment_x and inout are in HBM. */
int mdb_comoments_buckets_dev(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y,
                              const uint32_t *group_of_segment_x, const mdb_bucket_request *request,
                              mdb_comoments_cell *inout);
/* Several host batches per field (rows in the order of each list) folded as one batch per field; group_of_segment_x:
 * one array per batch of xs, or NULL. */
int mdb_comoments_buckets_list(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                               uint32_t n_y, const uint32_t *const *group_of_segment_x,
                               const mdb_bucket_request *request, mdb_comoments_cell *inout);
/* Host arithmetic, no context, no GPU: into[j] merged with from[j] by the merge rule, for j < n. */
int mdb_comoments_merge_n(mdb_comoments_cell *into, const mdb_comoments_cell *from, uint64_t n);
/* Host arithmetic, no context, no GPU: out[j] = (count, mean, m2) of field `which` (0: x, 1: y) of cells[j]. */
int mdb_comoments_moments(const mdb_comoments_cell *cells, uint64_t n, uint32_t which, mdb_moments_cell *out);
/* Host arithmetic, no context, no GPU: out[j] = the MDB_COMOMENTS_* statistic `kind` of cells[j] (NaN as listed). */
int mdb_comoments_finish(const mdb_comoments_cell *cells, uint64_t n, uint32_t kind, double *out);

/* Extension: DERIVED FIELDS of two fields - the generated column z = f(x, y) and, per date_bin bucket and group, its
 * count, mean, m2, MIN and MAX:
 *   power = voltage * current, dT = outlet - inlet, efficiency = output / input, |forecast - actual| (MAE, largest error)
 * A generated field FIELD AS (column_one + column_two) is answered by the reference with GridExec per field ->
 * SortedJoinExec -> GeneratedAsExec -> AggregateExec (crates/modelardb_storage/src/query/generated_as_exec.rs; the
 * fields are zipped by row position, query/sorted_join_exec.rs:278-310): every point of both fields is rebuilt on the
 * host. Here both fields are rebuilt values-only into two scratch columns that live in HBM only, and the reduction
 * runs over ROWS, not over segments: a derived field needs every row of both fields whatever the model type.
 *   expr: mdb_derived_expr (mdb_format.h) - LINEAR, PRODUCT or RATIO with finite a, b, c and the optional ABS flag;
 *     binary32 operations in the written order, nothing fused, denormals kept, the correctly rounded division.
 *   x, y: two field columns of the same series with the same timestamps, each cut into segments in its own way (the
 *     alignment rule of the row masks); y may be the same batch as x.
 *   Which points: the rows of mdb_grid_batch_range(x, t_lo, t_hi) and of mdb_grid_batch_range(y, t_lo, t_hi), in
 *     order; row r of one is paired with row r of the other. Only the row COUNT under [t_lo, t_hi] is checked; a
 *     mismatch fails before anything is written, with a message that names both counts.
 *   mdb_derived_values*: values[r] = f(x[r], y[r]) for every row, timestamps[r] (or NULL) x's timestamp; *rows_out the
 *     row count. capacity smaller than the row count is an error that names the count. _dev: device batches and device
 *     outputs; values needs 4-byte alignment only, timestamps 16-byte alignment. The other form takes host batches and
 *     host outputs.
 *   mdb_derived_buckets*: request is mdb_bucket_request, unchanged; which_mask must be 0. inout: row-major
 *     [n_groups][n_buckets] cells (mdb_derived_cell, mdb_format.h); a fresh cell is all-zero bytes. A pair takes the
 *     bucket of its x-side timestamp and the group of its x-side segment, and is counted exactly where mdb_agg_buckets
 *     counts the x point for the same request: count equals that COUNT, always.
 *   How: per (x segment, bucket) pair the interval of rows it holds - O(1) on regular timestamps for every model type,
 *     one pass over the timestamps of a segment otherwise. An interval of at most MDB_DERIVED_SHORT_ROWS rows is reduced
 *     by one lane; a longer one is cut at the multiples of MDB_DERIVED_CHUNK_ROWS in absolute row numbers and one wave
 *     reduces each chunk with 16-byte loads of both columns. A run (an interval, or a lane's share of a chunk) is
 *     summed around its first z as mdb_moments_buckets sums a run; runs meet only through the merge rule.
 *   Merge rule, the same in mdb_derived_merge_n and in every kernel: count, mean and m2 as mdb_moments_merge_n; min and
 *     max by mdb_agg_buckets' rule for MIN and MAX (mdb_format.h: a NaN is skipped, -0.0 == +0.0 and the first one
 *     met stays - the sign of a zero extreme is the only thing about min and max that follows the order of merges); an
 *     empty side gives the other side's bytes. A cell of equal z has m2 == 0.0 and mean == z exactly, in any order of
 *     merges. A cell that receives no pair keeps every byte it had.
 *   Non-finite z: count is exact, min and max skip NaNs, and neither mean nor m2 is finite; nothing more is promised.
 *   Determinism: for the same input, request, expression and form two runs agree bit for bit, and so do the host, dev
 *     and list forms; no float atomics, no atomics on cells. MDB_AGG_BUCKET_SLICE_PAIRS, the order of the segments and
 *     cutting a batch into calls move mean and m2 by rounding only and never count, min or max.
 *   Scratch: the two columns take 8 B per row under [t_lo, t_hi]. Under mdb_set_scratch_limit columns larger than the
 *     limit are refused with a message that states the bytes needed: cut the batch by series, the cells merge.
 *   Errors (mdb_last_error set, inout and the outputs untouched - with one exception, that of mdb_grid_batch_range_dev:
 *     mdb_derived_values* lets the range grid of x write timestamps, and values where it is 16-byte aligned, in place,
 *     so a bit stream of x that turns out malformed only while it is decoded fails the call after rows have been
 *     written; everything the row plans find, and every error of y, whose grid runs first and into scratch, comes
 *     before the first store): those of mdb_moments_buckets*, a NULL y or expr, an
 *     unknown op or flag bit, a NaN or infinite a, b or c, the row-count mismatch, the columns refused, a capacity too
 *     small, a malformed segment in x or y. An empty batch, n_buckets == 0 or an empty range succeeds and changes
 *     nothing (*rows_out = 0). */
#define MDB_DERIVED_SHORT_ROWS 64u    /* an interval of at most this many rows: one lane */
#define MDB_DERIVED_CHUNK_ROWS 1024u  /* a longer one: one wave per chunk of this many rows */
int mdb_derived_values_dev(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const mdb_derived_expr *expr,
                           int64_t t_lo, int64_t t_hi, int64_t *timestamps, float *values, uint64_t capacity,
                           uint64_t *rows_out);
/* Host batches, host outputs. */
int mdb_derived_values(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const mdb_derived_expr *expr,
                       int64_t t_lo, int64_t t_hi, int64_t *timestamps, float *values, uint64_t capacity,
                       uint64_t *rows_out);
int mdb_derived_buckets(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const uint32_t *group_of_segment_x,
                        const mdb_bucket_request *request, const mdb_derived_expr *expr, mdb_derived_cell *inout);
/* All device pointers: both batches, group_of_segment_x and inout are in HBM (expr is a host pointer). */
int mdb_derived_buckets_dev(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y,
                            const uint32_t *group_of_segment_x, const mdb_bucket_request *request,
                            const mdb_derived_expr *expr, mdb_derived_cell *inout);
/* Several host batches per field (rows in the order of each list) folded as one batch per field; group_of_segment_x:
 * one array per batch of xs, or NULL. */
int mdb_derived_buckets_list(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                             uint32_t n_y, const uint32_t *const *group_of_segment_x,
                             const mdb_bucket_request *request, const mdb_derived_expr *expr, mdb_derived_cell *inout);
/* Host arithmetic, no context, no GPU: z[j] = f(x[j], y[j]) for j < n, by the evaluator the kernels use. */
int mdb_derived_apply(const mdb_derived_expr *expr, const float *x, const float *y, uint64_t n, float *z);
/* Host arithmetic, no context, no GPU: into[j] merged with from[j] by the merge rule, for j < n. */
int mdb_derived_merge_n(mdb_derived_cell *into, const mdb_derived_cell *from, uint64_t n);
/* Host arithmetic, no context, no GPU: out[j] = (count, mean, m2) of cells[j]: what mdb_moments_variance takes. */
int mdb_derived_stats(const mdb_derived_cell *cells, uint64_t n, mdb_moments_cell *out);

/* Extension: ROLLING WINDOWS over per-bucket cells - moving aggregates:
 *   a 1-hour moving average every minute, a rolling stddev or correlation, the 15-minute rolling maximum, energy over
 *   the trailing 24 hours every hour, avg_over_time(x[1h]) at a 1-minute step,
 *   f(...) OVER (ORDER BY bucket ROWS BETWEEN window-1 PRECEDING AND CURRENT ROW) on a downsampled series.
 * Every per-bucket operator answers tumbling buckets; a window of `window` buckets of width w is the merge of `window`
 * adjacent cells. The tumbling cells are computed once by the operator (unchanged) and rolled here with O(1) merges
 * per window whatever the window's length, in HBM for the _dev form: only the windows need to leave the device.
 *   request: mdb_roll_request (mdb_format.h): the kind (cell type and merge rule), the view [n_outer][n_buckets][n_inner]
 *     of the cells, window and stride in buckets.
 *   Windows: window k of a column (outer, inner) covers the buckets [k * stride, k * stride + window). Only whole
 *     windows exist: n_windows = n_buckets < window ? 0 : (n_buckets - window) / stride + 1 (mdb_roll_windows). A
 *     caller who wants trailing windows from its first instant on starts its buckets window - 1 widths earlier.
 *   out: row-major [n_outer][n_windows][n_inner] cells of the same type. Every cell of it is WRITTEN (not merged into).
 *   The rule - the ABI promises these bits, not a schedule. With m = window the buckets are cut into blocks of m,
 *     aligned at multiples of m from bucket 0:
 *       prefix  P_j[0] = cell[j*m],          P_j[i] = merge(into = P_j[i-1], from = cell[j*m+i])
 *       suffix  S_j[m-1] = cell[j*m+m-1],    S_j[i] = merge(into = a copy of cell[j*m+i], from = S_j[i+1])
 *     and for the window that starts at a = k * stride, j = a / m, r = a % m:
 *       r == 0: out = P_j[m-1] - the plain left fold, byte for byte what chaining the operator's *_merge_n over the m
 *               cells gives;            otherwise: out = merge(into = S_j[r], from = P_{j+1}[r-1]).
 *     merge is the operator's existing rule, unchanged: where it has an empty side that side yields the other's bytes,
 *     and a window over fresh cells only is a fresh cell.
 *   What follows: integer members are exact in any case. Float members differ from a direct call of the operator with
 *     buckets of width window * w by rounding only. mdb_roll_cells and mdb_roll_cells_dev agree bit for bit, and so do
 *     two runs. M4 windows are byte-identical to the direct call (its selection rules do not depend on the order). The
 *     sign of a zero MIN / MAX follows the left-to-right order of the buckets. MDB_ROLL_U64 adds wrapping. One thing
 *     is left open, as it is by the merge rules themselves: WHICH NaN a float member holds when it is one - the sign
 *     and payload are those of the instruction that added or multiplied (x86 makes another NaN of inf - inf than
 *     gfx950, and of two NaN operands either may come out); that the member is a NaN is part of the promise.
 *   Trend cells (mdb_trend_buckets*) are mdb_comoments_cell with mean_x relative to the cell's OWN bucket. Before they
 *     are rolled the caller adds b * width to mean_x of every non-empty cell of bucket b, and subtracts
 *     k * stride * width from every non-empty window k afterwards (exact in integers below 2^53); m2_x and c_xy, and
 *     with them slope, r2 and corr, do not depend on the shift.
 *   _dev: cells and out are in HBM and 8-byte aligned; the two launches (k_roll_suffix - not when stride is a multiple
 *     of window - and k_roll_windows) are enqueued on the context's stream, and the call returns without waiting for
 *     them. Scratch: the suffix folds, at most the bytes of the cells. Under mdb_set_scratch_limit a suffix array larger
 *     than the limit is refused with a message that states the bytes needed: cut the cells by n_outer.
 *   Errors (mdb_last_error set, out untouched, all found before the device is used): a NULL pointer; an unknown kind; a
 *     flag bit; window == 0 or stride == 0; n_outer * n_buckets * n_inner * the cell size overflowing 64 bits;
 *     capacity_cells below n_outer * n_windows * n_inner (the message names the count needed); out overlapping cells;
 *     _dev: a pointer that is not 8-byte aligned, the scratch refused. Any dimension 0, or n_buckets < window, succeeds
 *     and writes nothing.
 * Host arithmetic, no context, no GPU: the number of whole windows. */
int mdb_roll_windows(const mdb_roll_request *request, uint64_t *n_windows);
/* Host arithmetic, no context, no GPU: cells and out are host arrays. */
int mdb_roll_cells(const mdb_roll_request *request, const void *cells, void *out, uint64_t capacity_cells);
/* Device pointers: cells and out are in HBM. */
int mdb_roll_cells_dev(mdb_ctx *ctx, const mdb_roll_request *request, const void *cells, void *out,
                       uint64_t capacity_cells);

/* Extension: value histograms and exact quantiles PER BUCKET of date_bin(width, ts, origin) and group -
 *   SELECT date_bin(...), approx_percentile_cont(field, 0.95) ... GROUP BY 1 / median(field) per bucket / a heat map
 *   (time bucket x value cell),
 * which the reference answers with GridExec -> AggregateExec GROUP BY the date_bin, every point rebuilt first: its
 * model-based rule rewrites only count / min / max / sum / avg and only without a GROUP BY on time
 * (crates/modelardb_storage/src/optimizer/model_simple_aggregates.rs:319-323), so it rewrites neither the percentile
 * nor the grouping. mdb_hist_batch / mdb_quantile_batch answer it for ONE time range a call; these answer every bucket
 * in one call.
 *   request: mdb_bucket_request, unchanged; which_mask must be 0. group_of_segment as for mdb_agg_buckets.
 *   edges, cells: those of mdb_hist_batch - 1 .. MDB_HIST_MAX_EDGES edges, strictly increasing in totalOrder, the cell
 *     of a value = the number of edges at or below it; n_cells = n_edges + 1.
 *   counts: uint64_t [n_groups][n_buckets][n_cells], row-major. A call ADDS to them; a cell that receives nothing keeps
 *     its bytes; they are touched only once the pass is known to be free of errors.
 *   Which points: exactly those mdb_agg_buckets counts for the same request - bucket floor((t - origin) / width) in
 *     [0, n_buckets), t in [t_lo, t_hi], segment row i in group group_of_segment[i]. Per (group, bucket) the cells'
 *     increments add up to that operator's COUNT, always.
 *   Cost: one pass. PMC-Mean on regular timestamps is one addition per (segment, bucket); Swing on regular timestamps
 *     the binary searches of mdb_hist_batch per (segment, bucket); a stream of VALUES (MacaqueV, a residual tail) is
 *     decoded once however many buckets its segment reaches. Irregular TIMESTAMPS are decoded a constant number of
 *     times per pass, not once: once by the segment's analysis, once to place the points, and under values in a bit
 *     stream once more where a model precedes a residual tail (three times, so twelve per mdb_quantile_buckets call);
 *     such segments also take 8 bytes of scratch per bucket they reach. Only a malformed stream whose timestamps are
 *     not sorted is walked bucket by bucket.
 *   Determinism: integers only (integer atomics on zeroed scratch): the three forms and any two runs agree bit for
 *     bit.
 *   Errors (mdb_last_error set, counts untouched): a NULL argument; which_mask != 0; a bad edge list; width <= 0;
 *     n_groups == 0; n_groups * n_buckets * n_cells overflowing or not fitting the device's memory; a group id >=
 *     n_groups on ANY row, also one the request does not reach; a malformed segment among those the request reaches.
 *     An empty batch, n_buckets == 0 or an empty time range succeeds and changes nothing.
 *     "Not fitting" is judged against the device's TOTAL memory, as mdb_hist_batch does: counters between what is free
 *     and the total fail in the allocation instead, with the allocator's message - counts untouched either way. The
 *     same holds for the windows of mdb_quantile_buckets. */
int mdb_hist_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                     const mdb_bucket_request *request, const float *edges, uint32_t n_edges, uint64_t *counts);
/* The segments, group_of_segment and counts are in HBM; request and edges are host pointers. */
int mdb_hist_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                         const mdb_bucket_request *request, const float *edges, uint32_t n_edges, uint64_t *counts);
/* Several host batches (rows in the order of the list) counted as one batch; group_of_segment[k] (or NULL) per batch. */
int mdb_hist_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                          uint32_t n_inputs, const mdb_bucket_request *request, const float *edges, uint32_t n_edges,
                          uint64_t *counts);
/* Exact order statistics of every (group, bucket) cell, in totalOrder: out_lo / out_hi are float
 * [n_groups][n_buckets][n_q], n_points uint64_t [n_groups][n_buckets] (written for every cell). For a cell of N points
 * and q[i] in [0, 1]: p = q[i] * (double)(N - 1), out_lo = the floor(p)-th smallest point of the cell (0-based), out_hi
 * the ceil(p)-th (mdb_quantile_positions). A cell with N == 0 leaves its out_lo / out_hi entries untouched.
 * Interpolation is the caller's. 1 <= n_q <= MDB_QUANTILE_BUCKETS_MAX_Q.
 * How: a radix selection on the 32-bit keys, 8 + 8 + 8 + 8 bits, with a window of 256 counters per (cell, rank):
 * MDB_QUANTILE_BUCKETS_PASSES passes over the resident batch (the host form uploads it once) serve every cell and
 * every rank, whatever their number; the digit of a rank is chosen on the device, only n_points and the final keys
 * come back. Counters: n_groups * n_buckets * 2 n_q * 256 * 8 bytes of scratch. The cells of a later pass are narrow
 * (2^16, 2^8, then one key), so the closed form of a Swing segment on regular timestamps - binary searches per cell it
 * crosses - gives way to point-by-point evaluation there: a Swing segment costs O(points) per pass from the second
 * pass on, where the histogram costs O(cells crossed * log points).
 * Errors (outputs untouched): those of mdb_hist_buckets (without the edges; the counters are the windows), q outside
 * [0, 1] or NaN, n_q out of range. An empty batch writes n_points = 0 everywhere and nothing else. */
#define MDB_QUANTILE_BUCKETS_MAX_Q 4u
#define MDB_QUANTILE_BUCKETS_PASSES 4u
int mdb_quantile_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                         const mdb_bucket_request *request, const double *q, uint32_t n_q, float *out_lo, float *out_hi,
                         uint64_t *n_points);
/* The segments and group_of_segment are in HBM; the outputs are host pointers. */
int mdb_quantile_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                             const mdb_bucket_request *request, const double *q, uint32_t n_q, float *out_lo,
                             float *out_hi, uint64_t *n_points);

/* Extension: the moments of one field per VALUE CELL of another - per bucket of date_bin(width, ts, origin), group and
 * cell of x the count, the mean and m2 = the sum of (y - mean)^2 of the y values of the pairs whose x value falls in
 * the cell:
 *   SELECT width_bucket(wind_speed, ...), count(active_power), avg(active_power), stddev(active_power) ...
 *     GROUP BY 1 [, date_bin(...), turbine]
 * - the power curve of IEC 61400-12 (the "method of bins"), efficiency against load, a scatter plot reduced to a band.
 * The reference answers it with GridExec per field -> SortedJoinExec -> AggregateExec, every point of both fields
 * rebuilt. Here x is walked on its segments and contributes only the boundaries of its runs; y is the values-only
 * column of mdb_comoments_buckets (4 B per row, HBM only).
 *   Pairs: exactly those of mdb_comoments_buckets - row r of mdb_grid_batch_range(x, t_lo, t_hi) with row r of the same
 *     for y; a pair takes the bucket of its x-side timestamp and the group of its x-side segment. Rows outside buckets
 *     0 .. n_buckets-1 keep their row number and are not counted. Only the row COUNT under [t_lo, t_hi] is checked; a
 *     mismatch fails before anything is written, with a message that names both counts. The cuts of x and y need not
 *     coincide.
 *   Cell: that of mdb_hist_cell_of applied to the x value - 1 .. MDB_HIST_MAX_EDGES edges, strictly increasing in
 *     totalOrder, n_cells = n_edges + 1, the cell = the number of edges at or below the value's key. A NaN, a +-0 or an
 *     infinity of x lands where its key puts it.
 *   inout: mdb_moments_cell, row-major [n_groups][n_buckets][n_cells]; a fresh cell is all-zero bytes. A call MERGES
 *     into it; a cell that receives no pair keeps every byte it had. mdb_moments_merge_n and mdb_moments_variance take
 *     the cells unchanged. which_mask must be 0.
 *   How: a run is a maximal stretch of consecutive pairs of one x segment that stay in one bucket and one cell. It is
 *     summed around its first y value K: d = (double)y - (double)K, s1 += d, s2 += d * d; mean = K + s1 / n,
 *     m2 = s2 - s1 * s1 / n (0 where that rounds below 0). Runs meet only through the merge rule of
 *     mdb_moments_merge_n: a cell whose y values are all equal has m2 == 0.0 and mean == the value exactly, in any order
 *     of merges. PMC-Mean on regular timestamps is one run per bucket reached; Swing on regular timestamps the binary
 *     searches of mdb_hist_batch per bucket; a stream of values or timestamps is decoded a constant number of times
 *     per pass (two passes: one counts the runs, one reduces y over them), as mdb_hist_buckets does; only a malformed
 *     stream whose timestamps are not sorted is walked bucket by bucket. The batch's cursor index is not used.
 *   Invariants: count[g][b][c] equals what mdb_hist_buckets(x, the same request, the same edges) adds, exactly and
 *     always; its sum over c equals the COUNT of mdb_agg_buckets(x); the cells of a (group, bucket) folded over c with
 *     mdb_moments_merge_n give, within the moments' tolerance, the y moments of mdb_comoments_buckets(x, y).
 *   Non-finite y: in a cell that holds a NaN or an infinity of y count is exact and neither mean nor m2 is finite;
 *     nothing more is promised. A non-finite x only decides the cell.
 *   Determinism, as for mdb_moments_buckets: for the same input, request, edges and form two runs agree bit for bit,
 *     and so do the host, dev and list forms; no float atomics, no atomics on cells. MDB_AGG_BUCKET_SLICE_PAIRS, the
 *     order of the segments, cutting a batch into calls and whether the keys had to be sorted move mean and m2 by
 *     rounding only.
 *   Scratch: the y column takes 4 B per row under [t_lo, t_hi] (refused under mdb_set_scratch_limit as for
 *     mdb_comoments_buckets); a run takes 32 B, the cell and its 8-byte key; 16 B per segment of x for the run counts
 *     and offsets, which are also read back once (8 B per segment) to cut the slices. On an x field whose noise crosses
 *     an edge at every point runs approach points. Slices of at most MDB_AGG_BUCKET_SLICE_PAIRS runs are folded one
 *     after the other; a slice ends only at a segment boundary, so a single segment with more runs than that is a slice
 *     of its own and needs 32 B for each of its runs (at most 2^31 runs in one segment).
 *   Errors (mdb_last_error set, inout untouched): those of mdb_comoments_buckets* - a NULL argument, a NULL y, the
 *     row-count mismatch, the y column refused, a malformed segment in x or y - and those of mdb_hist_buckets*: a bad
 *     edge list, n_groups * n_buckets * n_cells overflowing or not fitting the device's memory, a group id >= n_groups
 *     on ANY row. What can be checked without the device is checked before it is used. An empty batch, n_buckets == 0
 *     or an empty time range succeeds and changes nothing. */
int mdb_binned_buckets(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const uint32_t *group_of_segment_x,
                       const mdb_bucket_request *request, const float *edges, uint32_t n_edges, mdb_moments_cell *inout);
/* Both batches, group_of_segment_x and inout are in HBM; request and edges are host pointers. */
int mdb_binned_buckets_dev(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y,
                           const uint32_t *group_of_segment_x, const mdb_bucket_request *request, const float *edges,
                           uint32_t n_edges, mdb_moments_cell *inout);
/* Several host batches per field (rows in the order of each list) folded as one batch per field; group_of_segment_x:
 * one array per batch of xs, or NULL. */
int mdb_binned_buckets_list(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                            uint32_t n_y, const uint32_t *const *group_of_segment_x,
                            const mdb_bucket_request *request, const float *edges, uint32_t n_edges,
                            mdb_moments_cell *inout);

/* Extension: the linear trend of a field over TIME - per bucket of date_bin(width, ts, origin) and group one
 * mdb_comoments_cell with x = the time offset of the point inside its bucket and y = its value:
 *   SELECT turbine, date_bin(...), regr_slope(bearing_temp, ts), regr_r2(bearing_temp, ts), corr(bearing_temp, ts)
 *   ... GROUP BY 1, 2
 * mdb_comoments_buckets* cannot answer this: its y is a second field column of segments, and a timestamp is not one
 * (it does not fit an f32). The reference answers with GridExec -> AggregateExec over every rebuilt point. Here the
 * time side needs no data: on regular timestamps the sums of x over a run of n points are closed forms in n and the
 * sampling interval, a PMC-Mean segment gives its whole cell per bucket in O(1), a Swing segment needs only its values
 * point by point in registers. No y column, no scratch beyond the pairs.
 *   request: mdb_bucket_request, unchanged; which_mask must be 0. inout: row-major [n_groups][n_buckets] cells
 *     (mdb_comoments_cell, mdb_format.h); a fresh cell is all-zero bytes. A call MERGES into it.
 *   Which points: exactly those mdb_moments_buckets* counts for the same batch, groups and request; the checks, the
 *     errors and "inout untouched on error" are the same.
 *   x: for a counted point with timestamp t in bucket b, x = (double)(uint64_t)((t - origin) - b * width): it lies in
 *     [0, width), is formed in wrapping-exact integer arithmetic and converted once; exact below 2^53. x is relative
 *     to the bucket so that f64 keeps every digit at any epoch. regr_slope, corr, regr_r2 and covar_* do not depend on
 *     a shift of x: they are SQL's values for (field, ts). MDB_COMOMENTS_REGR_INTERCEPT is the fitted value at the
 *     bucket's first instant (what a chart needs); SQL's regr_intercept(field, ts) is that minus
 *     slope * (origin + b * width) - at epoch scale that subtraction cancels, whoever performs it.
 *   y: (double)v. count, mean_y and m2_y are the moments of the field.
 *   Run rule: a run (the points of one segment in one bucket, or of one piece of a stream in one bucket) is summed
 *     around its first pair as for mdb_comoments_buckets, with dx = the integer difference t - t_first converted to
 *     double (k * delta on regular timestamps). Runs meet only in the merge rule of mdb_comoments_merge_n.
 *     On regular timestamps n points at x0 + k * delta have mean_x = x0 + delta * (n-1)/2 and
 *     m2_x = delta^2 * n(n^2-1)/12; a PMC-Mean run adds mean_y = v and m2_y = c_xy = v - v.
 *   Merge and finish: mdb_comoments_merge_n, mdb_comoments_moments and mdb_comoments_finish, unchanged; x is the
 *     independent variable already.
 *   Exact promises: count equals mdb_agg_buckets' COUNT, always. A cell whose values are all equal and finite has
 *     m2_y == 0.0, c_xy == 0.0 and, with two or more distinct timestamps, slope == 0.0 exactly. A cell of one point, or
 *     of points that all share one timestamp, has m2_x == 0.0: the regr_* and corr kinds give NaN. A NaN or an infinity
 *     among the values makes mean_y, m2_y and c_xy non-finite; mean_x and m2_x stay finite and correct.
 *   Determinism, as for mdb_moments_buckets: two runs and the three forms agree bit for bit; the order of segments,
 *     the cut of batches and MDB_AGG_BUCKET_SLICE_PAIRS move the five doubles by rounding only.
 *   Origin invariance: moving the origin by a whole number of widths, with n_buckets moved along, gives the same bytes
 *     in the cells that still exist.
 *   Time unit: microseconds, as mdb_bucket_request states; the slope is per microsecond.
 *   Errors (mdb_last_error set, inout untouched): those of mdb_moments_buckets*. An empty batch or n_buckets == 0
 *     succeeds and changes nothing. */
int mdb_trend_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                      const mdb_bucket_request *request, mdb_comoments_cell *inout);
/* All device pointers: the batch, group_of_segment and inout are in HBM. */
int mdb_trend_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                          const mdb_bucket_request *request, mdb_comoments_cell *inout);
/* Several host batches (rows in the order of the list) folded as one batch; group_of_segment: one array per batch, or NULL. */
int mdb_trend_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                           uint32_t n_inputs, const mdb_bucket_request *request, mdb_comoments_cell *inout);

/* Extension: EPISODES - the maximal runs of points that pass a value predicate: when was bearing_temp > 85, for how
 * long each time, and how bad was it. In SQL the gaps-and-islands pattern (lag() over the filtered rows, GROUP BY
 * island), for which the reference rebuilds every point (GridExec -> FilterExec -> WindowAggExec -> AggregateExec).
 * Here a segment is summarised in O(1) (PMC-Mean) or two binary searches (Swing), the summaries are stitched by a
 * device-wide scan, and only the episodes leave the device.
 *   Rows: those of mdb_grid_batch_range(in, filter.t_lo, filter.t_hi), in that order - the row numbering of the
 *     masks. Row r has timestamp ts(r), value v(r), segment row seg(r) and group g(r) = group_of_segment[seg(r)]
 *     (group_of_segment NULL: 0).
 *   Passing: row r passes iff v(r) passes the filter's value bounds in totalOrder: the set bits of mdb_mask_filter_dev.
 *   Continuing: row r >= 1 continues row r-1 iff g(r) == g(r-1) and ts(r) >= ts(r-1) and ts(r) - ts(r-1) <= max_gap
 *     (the difference formed as uint64_t after the comparison). The rule holds for every pair of consecutive rows,
 *     inside a segment or across segments: a step backwards in time ends an episode, as when the next series
 *     begins. max_gap == INT64_MAX switches the gap rule off.
 *   Episode: a maximal set of consecutive rows that all pass, each but the first continuing its predecessor;
 *     reported iff count >= min_count and t_last - t_first >= min_duration. Episodes come out ordered by first_row.
 *   Exact promises: every field but `sum` is exact; sum is the f64 sum of the f32 values within 0.001 % of the sum
 *     of their magnitudes. With both minimum filters off the episodes are disjoint and the union of
 *     [first_row, first_row + count) is exactly the set bits of mdb_mask_filter_dev. An episode of equal finite
 *     values has min == max == that value.
 *   Determinism: for the same input, request and form two runs agree byte for byte, and the four forms agree byte
 *     for byte; no float atomics, and no grouping of f64 additions depends on timing. MDB_FILTER_SLICE_POINTS may
 *     move `sum` by rounding only.
 *   Errors (mdb_last_error set, outputs untouched): a NULL argument, unknown filter flag bits or reserved != 0,
 *     flags != 0, a negative max_gap or min_duration, n_groups == 0, a group id >= n_groups on ANY segment of the
 *     batch (inside the time range or not), a too small cap, the error classes of the range calls. What can be
 *     checked without the device is checked before the device is used. An empty batch, an empty time range and an
 *     empty value interval are valid and give no episode. */
typedef struct mdb_episode {      /* 64 bytes */
    uint64_t first_row;           /* row number as defined above */
    uint64_t count;               /* rows first_row .. first_row + count - 1 */
    int64_t  t_first, t_last;
    double   sum;                 /* f64 sum of the f32 values */
    float    min, max;            /* as mdb_agg_state folds them: fmin / fmax from FLT_MAX / -FLT_MAX, a NaN is skipped */
    uint32_t group;
    uint32_t first_segment;       /* segment row of the batch (of the list) that holds first_row */
    uint64_t reserved;            /* 0 */
} mdb_episode;

typedef struct mdb_episodes_request {   /* 64 bytes */
    mdb_value_filter filter;
    int64_t  max_gap;             /* >= 0 */
    int64_t  min_duration;        /* >= 0 */
    uint64_t min_count;           /* 0 and 1: every episode */
    uint32_t n_groups;            /* >= 1 */
    uint32_t flags;               /* must be 0 */
} mdb_episodes_request;

typedef struct mdb_episodes_result {
    mdb_episode *episodes;        /* host memory, n of them (NULL if n == 0) */
    uint64_t n, n_rows, n_passing;
    void *priv_;
} mdb_episodes_result;

MDB_LAYOUT_ASSERT(sizeof(mdb_episode) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_episode, sum) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_episode, min) == 40);
MDB_LAYOUT_ASSERT(offsetof(mdb_episode, group) == 48);
MDB_LAYOUT_ASSERT(offsetof(mdb_episode, reserved) == 56);
MDB_LAYOUT_ASSERT(sizeof(mdb_episodes_request) == 64);
MDB_LAYOUT_ASSERT(offsetof(mdb_episodes_request, max_gap) == 32);
MDB_LAYOUT_ASSERT(offsetof(mdb_episodes_request, n_groups) == 56);

/* The batch and group_of_segment (may be NULL) in HBM. n_rows: the rows under the time range; n_passing: the passing
 * ones (the sum of the count fields only when both minimum filters are off). */
int mdb_episodes_count_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                           const mdb_episodes_request *request, uint64_t *n_episodes, uint64_t *n_rows,
                           uint64_t *n_passing);
/* ... and the episodes into out (HBM, room for cap of them). A too small cap fails and writes nothing. */
int mdb_episodes_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                     const mdb_episodes_request *request, mdb_episode *out, uint64_t cap, uint64_t *n_out,
                     uint64_t *n_rows, uint64_t *n_passing);
/* Host batch and host group_of_segment (may be NULL); only the episodes cross PCIe on the way back. */
int mdb_episodes(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                 const mdb_episodes_request *request, mdb_episodes_result **out);
/* Several host batches (rows in the order of the list) folded as one batch: an episode may cross from one input to
 * the next, first_segment counts through the list. group_of_segment: one array per batch, or NULL. */
int mdb_episodes_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                      uint32_t n_inputs, const mdb_episodes_request *request, mdb_episodes_result **out);
void mdb_episodes_result_free(mdb_episodes_result *result);

/* Extension: TIME-WEIGHTED averages and integrals per bucket of date_bin(width, ts, origin) and group - the series
 * taken as a function of time, not as a set of points: energy = integral of power, the share of a window a setpoint
 * was held, degree-hours. Elsewhere time_weight('Linear' | 'LOCF', ts, v) / integral(), or lag() over every rebuilt
 * point followed by a weighted sum (GridExec -> WindowAggExec -> AggregateExec). Here a PMC-Mean segment's share of a
 * bucket is value x clipped duration, a Swing segment's a closed form of its line, both O(1) per (segment, bucket).
 *   request: mdb_integral_request (mdb_format.h). buckets.t_lo / t_hi must be INT64_MIN / INT64_MAX and which_mask 0:
 *     the buckets are the range. inout: row-major [n_groups][n_buckets] mdb_integral_cell; a fresh cell is all-zero
 *     bytes. A call MERGES into it.
 *   Rows: those of mdb_grid_batch(in), in that order; no time range applies. Row r has ts(r), v(r) and
 *     g(r) = group_of_segment[seg(r)] (NULL: 0).
 *   Linked: rows r and r+1 are linked iff g(r+1) == g(r) and ts(r+1) > ts(r) and ts(r+1) - ts(r) <= max_gap (the
 *     difference formed as uint64_t after the comparison). The rule holds for every pair of consecutive rows, inside a
 *     segment and across segments - and, in the list form, across inputs. It does not hold across separate calls: cut
 *     batches at series boundaries. A regular segment whose sampling interval exceeds max_gap has no linked pair inside
 *     it. A segment that rebuilds to no row (end_time < start_time) links nothing across it.
 *   The function: on a linked interval [t0, t1] with values v0, v1, MDB_INTEGRAL_LINEAR is
 *     f(t) = v0 + (v1 - v0)(t - t0)/(t1 - t0), MDB_INTEGRAL_STEP is f(t) = v0. Outside linked intervals the series is
 *     undefined and contributes nothing.
 *   The cell: bucket b is [origin + b*width, origin + (b+1)*width). For every linked interval, a = max(t0, bucket
 *     start), e = min(t1, bucket end); if e > a, duration += e - a (an integer number of microseconds) and integral +=
 *     the integral of f over [a, e] in value x microseconds, an f64 formed from integer time differences converted
 *     once. An interval may cross any number of bucket edges and either of its points may lie outside every bucket;
 *     nothing overflows for any origin or width.
 *   Finish: mdb_integral_average writes integral / duration, NaN where duration == 0. mdb_integral_merge_n adds both
 *     members.
 *   Exact promises: duration is exact, always - also beside NaN and infinite values; over buckets that cover a group's
 *     rows the durations sum to the group's linked time. A cell whose contributing values are all one finite c has an
 *     average within 2^-44 |c| of c. LINEAR: a non-finite v0 or v1 makes the integral of the cells its interval
 *     touches non-finite; STEP: only a non-finite v0 does.
 *   Tolerance: |integral - exact| <= 1e-5 x the sum of (e - a) max(|v0|, |v1|) over the cell's pieces.
 *   Determinism: two runs and the three forms agree bit for bit; no float atomics. The order of segments and
 *     MDB_AGG_BUCKET_SLICE_PAIRS move integral by rounding only, duration not at all. Moving the origin by a whole
 *     number of widths, with n_buckets moved along, gives the same bytes.
 *   Errors (mdb_last_error set, inout untouched; what needs no device is checked before the device is used): a NULL
 *     argument, width <= 0, n_groups == 0, an overflowing cell count, which_mask != 0, a time range in the bucket
 *     request, an unknown method, flags != 0, a negative max_gap, a group id >= n_groups on ANY row, the
 *     malformed-segment classes of mdb_agg_buckets for the segments the request reaches and the neighbour whose first
 *     point it reads. An empty batch or n_buckets == 0 succeeds and changes nothing. */
int mdb_integral_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                         const mdb_integral_request *request, mdb_integral_cell *inout);
/* All device pointers: the batch, group_of_segment and inout are in HBM. */
int mdb_integral_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                             const mdb_integral_request *request, mdb_integral_cell *inout);
/* Several host batches (rows in the order of the list) folded as one batch: a linked interval may cross from one input
 * to the next. group_of_segment: one array per batch, or NULL. */
int mdb_integral_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                              uint32_t n_inputs, const mdb_integral_request *request, mdb_integral_cell *inout);
/* into[k] += from[k] for k < n, both members. Host memory, no context. */
int mdb_integral_merge_n(mdb_integral_cell *into, const mdb_integral_cell *from, uint64_t n);
/* out[k] = cells[k].integral / cells[k].duration, NaN where duration == 0. Host memory, no context. */
int mdb_integral_average(const mdb_integral_cell *cells, uint64_t n, double *out);

/* Extension: the value of a series AT REGULAR INSTANTS - gap-fill, last observation carried forward, interpolation.
 * Elsewhere time_bucket_gapfill(...) with locf() / interpolate(), or resample().ffill() / .interpolate(); it is also
 * how two fields that do not share timestamps are brought to one time axis. Here a PMC-Mean or Swing segment on regular
 * timestamps gives the value at any instant inside it in O(1), one lane per (segment, instant), and 16 bytes per
 * instant leave the device however many points lie between two instants.
 *   request: mdb_sample_request (mdb_format.h). Instant k is origin + k*width for k < n_buckets. instants.t_lo / t_hi
 *     must be INT64_MIN / INT64_MAX and which_mask 0. inout: row-major [n_groups][n_instants] mdb_sample_cell; a fresh
 *     cell is all-zero bytes. A call MERGES into it.
 *   Rows: those of mdb_grid_batch(in), in that order. Row r has ts(r), v(r) and g(r) = group_of_segment[seg(r)]
 *     (NULL: 0).
 *   Linked: exactly the rule of mdb_integral_buckets - rows r and r+1 are linked iff g(r+1) == g(r) and ts(r+1) > ts(r)
 *     and ts(r+1) - ts(r) <= max_gap; inside segments, across segments, across the inputs of the list form; not across
 *     calls.
 *   Contributions at instant T, to cell (group, k):
 *     (a) every row with ts(r) == T contributes v(r);
 *     (b) under MDB_SAMPLE_LINEAR and MDB_SAMPLE_STEP every linked interval (t0, v0) - (t1, v1) with t0 < T < t1
 *         contributes f(T): STEP f = v0; LINEAR f = v0 when v0 == v1, else
 *         (double)v0 + ((double)v1 - (double)v0) * ((double)(T - t0) / (double)(t1 - t0)), the time differences formed
 *         in uint64_t and converted once. MDB_SAMPLE_EXACT has no (b).
 *     Each contribution adds 1 to count and its value, as f64, to sum. An instant nothing reaches keeps its cell
 *     untouched: that is the gap of gap-fill.
 *   Finish: mdb_sample_values writes sum / count, NaN where count == 0. mdb_sample_merge_n merges cells.
 *   Exact promises: count is exact, always - also beside NaN and infinite values. A cell with count == 1 holds sum ==
 *     that one contribution bit for bit (a cell that has received nothing takes its first contribution whole), so one
 *     series sampled on its own grid gives the float of mdb_grid_batch exactly under all three methods. A contribution
 *     that reads a non-finite value makes sum non-finite: LINEAR reads v0 or v1, STEP and rows read v0.
 *   Tolerance: |sum - exact| <= 2^-48 x the sum of max(|v0|, |v1|) over the cell's contributions: one contribution
 *     carries four roundings of at most 2^-53 on magnitudes up to 2 max(|v0|, |v1|), each addition of a cell 2^-53 of
 *     the running sum; the rest is margin for contraction and the order of additions.
 *   Determinism: two runs and the three forms agree bit for bit; no float atomics. MDB_AGG_BUCKET_SLICE_PAIRS and the
 *     order of segments move sum by rounding only, and only in cells with count > 1; count never moves. Moving the
 *     origin by a whole number of widths, with n_buckets moved along, gives the same bytes. Nothing overflows for any
 *     origin, width or timestamp; instants a real timestamp cannot reach are never formed.
 *   Errors (mdb_last_error set, inout untouched; what needs no device is checked before the device is used): a NULL
 *     argument, width <= 0, n_groups == 0, an overflowing cell count, which_mask != 0, a time range in the request, an
 *     unknown method, flags != 0, a negative max_gap, a group id >= n_groups on ANY row, the malformed-segment classes
 *     of mdb_agg_buckets for the segments the request reaches and the neighbour whose first point it reads. An empty
 *     batch or n_buckets == 0 succeeds and changes nothing. */
int mdb_sample_at(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                  const mdb_sample_request *request, mdb_sample_cell *inout);
/* All device pointers: the batch, group_of_segment and inout are in HBM. */
int mdb_sample_at_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                      const mdb_sample_request *request, mdb_sample_cell *inout);
/* Several host batches (rows in the order of the list) sampled as one batch: a linked interval may cross from one
 * input to the next. group_of_segment: one array per batch, or NULL. */
int mdb_sample_at_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                       uint32_t n_inputs, const mdb_sample_request *request, mdb_sample_cell *inout);
/* into[k] merged with from[k] for k < n: a cell with count == 0 takes the other whole, else both members are added.
 * Host memory, no context. */
int mdb_sample_merge_n(mdb_sample_cell *into, const mdb_sample_cell *from, uint64_t n);
/* out[k] = cells[k].sum / cells[k].count, NaN where count == 0. Host memory, no context. */
int mdb_sample_values(const mdb_sample_cell *cells, uint64_t n, double *out);

/* Extension: the CHANGES between consecutive points per bucket of date_bin(width, ts, origin) and group - how much a
 * counter grew and how often it restarted (increase() / rate() / resets(), non_negative_difference()), the largest
 * step up and down of a window (ramp rates, spikes), how much a signal moved at all (total variation). In SQL
 * v - lag(v) OVER (PARTITION BY series ORDER BY ts) followed by GROUP BY date_bin(...): GridExec -> WindowAggExec ->
 * AggregateExec over every rebuilt point. Here every step inside a PMC-Mean segment is zero, so a (segment, bucket)
 * pair is a count and a duration in O(1); a Swing segment's rows are arithmetic in registers; 64 bytes per cell leave
 * the device.
 *   request: mdb_change_request (mdb_format.h). buckets.t_lo / t_hi must be INT64_MIN / INT64_MAX and which_mask 0:
 *     the buckets are the range. inout: row-major [n_groups][n_buckets] mdb_change_cell; a fresh cell is all-zero
 *     bytes. A call MERGES into it.
 *   Rows: those of mdb_grid_batch(in), in that order; no time range applies. Row r has ts(r), v(r) and
 *     g(r) = group_of_segment[seg(r)] (NULL: 0).
 *   Linked: exactly the rule of mdb_integral_buckets - rows r and r+1 are linked iff g(r+1) == g(r) and ts(r+1) > ts(r)
 *     and ts(r+1) - ts(r) <= max_gap; inside segments, across segments, across the inputs of the list form; not across
 *     calls. A segment that rebuilds to no row (end_time < start_time) links nothing across it.
 *   The cell: a linked pair belongs to the bucket of its LATER row, (g, floor((ts(r+1) - origin) / width)), and is
 *     never cut; if ts(r+1) lies outside [origin, origin + n_buckets*width) the pair is dropped, ts(r) may lie
 *     anywhere. So the cells of adjacent buckets add up to the cell of their union, and the net change of a fully
 *     linked stretch telescopes to its last value minus the value before its first row. Per pair, with
 *     d = (double)v1 - (double)v0 (one rounding): count += 1 and duration += ts(r+1) - ts(r) (uint64_t, microseconds),
 *     always; d > 0: rise += d, max_rise = max(max_rise, d); d < 0: n_fall += 1, fall += -d, reset_sum += (double)v1,
 *     max_fall = max(max_fall, -d); d NaN (a NaN value, or inf - inf): rise += NaN and fall += NaN, the other members
 *     as for d == 0, which touches only count and duration.
 *   Finish: mdb_change_finish writes, per cell, MDB_CHANGE_NET rise - fall, MDB_CHANGE_VARIATION rise + fall,
 *     MDB_CHANGE_INCREASE rise + reset_sum, MDB_CHANGE_RATE (rise + reset_sum) * 1e6 / duration (the increase per
 *     second); NaN where count == 0, and for RATE also where duration == 0. mdb_change_merge_n adds the three integers
 *     and the three sums and takes the larger of each maximum.
 *   Exact promises: count, n_fall and duration are exact, always - also beside NaN and infinite values. max_rise and
 *     max_fall are bit-exact: each is a maximum of individually rounded differences, which no order moves. A cell
 *     whose rows all have one value has rise == fall == reset_sum == max_rise == max_fall == 0.0 exactly. A
 *     non-decreasing stretch has n_fall == 0 and fall == 0.0 exactly.
 *   Tolerance: for each of rise, fall and reset_sum, |got - exact| <= count * 2^-52 * S, S the sum of the magnitudes
 *     of the member's terms in the cell: one rounding of 2^-53 per term, and at most (n-1) * 2^-53 * S for adding n
 *     terms in any order through slices, tree and fold.
 *   Determinism: two runs and the three forms agree bit for bit; no float atomics. MDB_AGG_BUCKET_SLICE_PAIRS and the
 *     order of segments move the three sums by rounding only, the five other members not at all. Moving the origin by
 *     a whole number of widths, with n_buckets moved along, gives the same bytes as long as the buckets added or
 *     dropped hold no pair; where they do, the (segment, bucket) pairs in front of a cell's run change, the reduction
 *     cuts the run elsewhere and the three sums move by rounding. Nothing overflows for any origin, width or
 *     timestamp.
 *   Errors (mdb_last_error set, inout untouched; what needs no device is checked before the device is used): a NULL
 *     argument, width <= 0, n_groups == 0, an overflowing cell count, which_mask != 0, a time range in the bucket
 *     request, reserved != 0, flags != 0, a negative max_gap, a group id >= n_groups on ANY row, the malformed-segment
 *     classes of mdb_agg_buckets for the segments the request reaches and the neighbour whose first point it reads. An
 *     empty batch or n_buckets == 0 succeeds and changes nothing. */
int mdb_change_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                       const mdb_change_request *request, mdb_change_cell *inout);
/* All device pointers: the batch, group_of_segment and inout are in HBM. */
int mdb_change_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                           const mdb_change_request *request, mdb_change_cell *inout);
/* Several host batches (rows in the order of the list) folded as one batch: a linked pair may cross from one input to
 * the next. group_of_segment: one array per batch, or NULL. */
int mdb_change_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                            uint32_t n_inputs, const mdb_change_request *request, mdb_change_cell *inout);
/* into[k] merged with from[k] for k < n: integers and sums added, the larger of each maximum. Host memory, no context. */
int mdb_change_merge_n(mdb_change_cell *into, const mdb_change_cell *from, uint64_t n);
/* out[k] = the MDB_CHANGE_* `kind` of cells[k] (above); an unknown kind is an error. Host memory, no context. */
int mdb_change_finish(const mdb_change_cell *cells, uint64_t n, uint32_t kind, double *out);

/* Extension: the TIME SPENT per value cell, per bucket of date_bin(width, ts, origin) and group - time in state, a
 * load-duration curve, "the share of the day the rotor ran between 12 and 14 rpm", time above a limit per shift.
 * Elsewhere state_agg / duration_in, a time-weighted histogram, or lag() over every rebuilt point followed by GROUP BY
 * date_bin, width_bucket (GridExec -> WindowAggExec -> AggregateExec). mdb_hist_buckets counts points per value cell
 * and mdb_integral_buckets integrates over time; this is the product of the two. A PMC-Mean segment on regular
 * timestamps gives its share of a bucket in O(1), a Swing segment by the binary searches of mdb_hist_buckets.
 *   request: mdb_dwell_request (mdb_format.h). buckets.t_lo / t_hi must be INT64_MIN / INT64_MAX and which_mask 0:
 *     the buckets are the range. method must be MDB_DWELL_STEP, flags 0.
 *   edges, cells: those of mdb_hist_buckets - 1 .. MDB_HIST_MAX_EDGES edges, strictly increasing in totalOrder; the
 *     cell of a value is mdb_hist_cell_of; n_cells = n_edges + 1.
 *   dwell: row-major uint64_t [n_groups][n_buckets][n_cells], microseconds. A call ADDS to it.
 *   Rows and Linked: exactly those of mdb_integral_buckets - rows r and r+1 of mdb_grid_batch(in) are linked iff
 *     g(r+1) == g(r) and ts(r+1) > ts(r) and ts(r+1) - ts(r) <= max_gap; inside segments, across segments, across the
 *     inputs of the list form; not across calls. A segment that rebuilds to no row links nothing across it.
 *   The cell: on a linked interval (t0, v0) - (t1, v1) the series holds v0 on [t0, t1). For every bucket b, with
 *     a = max(t0, bucket start) and e = min(t1, bucket end): if e > a, dwell[g][b][cell_of(v0)] += e - a. An interval
 *     may cross any number of bucket edges; bucket ends saturate at INT64_MAX. v1 is never read; the last row of a
 *     linked run holds nothing. A non-finite v0 is placed by its totalOrder key like any other value: +NaN in the last
 *     cell, -NaN in the first, -0.0 below an edge at +0.0.
 *   Only STEP: under linear interpolation the instant at which a line crosses an edge is not an integer number of
 *     microseconds, and nothing below would be exact. MDB_INTEGRAL_LINEAR's number (0) is refused by name, not
 *     approximated.
 *   Exact promises: everything is integer microseconds, so every number is exact. The cells of a (group, bucket) row
 *     sum to mdb_integral_buckets' duration under MDB_INTEGRAL_STEP for the same request. Merging adjacent cells
 *     gives the cells of the coarser edge list; adjacent buckets add up to the bucket of their union.
 *   Determinism: integer atomics only; two runs and the three forms agree byte for byte, whatever the order of
 *     segments or the cut of batches at series boundaries. Moving the origin by whole widths, with n_buckets moved
 *     along, gives the same numbers.
 *   Finish: mdb_dwell_share writes dwell / (sum over the row's cells) as f64, NaN where the sum is 0;
 *     mdb_dwell_merge_n adds two arrays.
 *   Errors (mdb_last_error set, dwell untouched; what needs no device is checked before the device is used): a NULL
 *     argument, a bad edge list, width <= 0, n_groups == 0, an overflowing or non-fitting counter array, a time range
 *     in the request, which_mask != 0, an unknown method, flags != 0, a negative max_gap, a group id >= n_groups on ANY
 *     row, the malformed-segment classes of mdb_agg_buckets for the segments the request reaches. Of a segment's right
 *     neighbour only start_time, the group and whether it rebuilds to a row are read, the last from its views and times
 *     alone: a malformed neighbour that no bucket reaches is NOT reported (mdb_integral_buckets reads its first point
 *     and fails on it) and counts as a segment with rows, unless its timestamps' length is negative. On such a batch
 *     the promise about mdb_integral_buckets' duration is void: that call fails. An empty batch or n_buckets == 0
 *     succeeds and changes nothing. */
int mdb_dwell_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                      const mdb_dwell_request *request, const float *edges, uint32_t n_edges, uint64_t *dwell);
/* All device pointers but request and edges: the batch, group_of_segment and dwell are in HBM. */
int mdb_dwell_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                          const mdb_dwell_request *request, const float *edges, uint32_t n_edges, uint64_t *dwell);
/* Several host batches (rows in the order of the list) folded as one batch: a linked interval may cross from one input
 * to the next. group_of_segment: one array per batch, or NULL. */
int mdb_dwell_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                           uint32_t n_inputs, const mdb_dwell_request *request, const float *edges, uint32_t n_edges,
                           uint64_t *dwell);
/* into[k] += from[k] for k < n. Host memory, no context. */
int mdb_dwell_merge_n(uint64_t *into, const uint64_t *from, uint64_t n);
/* out[row * n_cells + c] = dwell[row * n_cells + c] / (the sum of the row's n_cells cells) for row < n_rows, NaN where
 * that sum is 0. Host memory, no context. */
int mdb_dwell_share(const uint64_t *dwell, uint64_t n_rows, uint32_t n_cells, double *out);

/* Extension: the TRANSITIONS between value cells, per bucket of date_bin(width, ts, origin) and group - how often the
 * series went from one band to another: starts per day of a machine (stopped -> running), upward crossings of a limit
 * per shift, the state-transition matrix of an operating mode. Elsewhere the transitions half of state_agg, a
 * level-crossing count, or lag() over every rebuilt point followed by GROUP BY date_bin, width_bucket(lag_v),
 * width_bucket(v) (GridExec -> WindowAggExec -> AggregateExec). mdb_dwell_buckets is the time half of that question,
 * mdb_change_buckets counts falls of any size and not crossings of a level. Inside a PMC-Mean segment every pair stays
 * in its cell, O(1) per bucket; along a Swing line the cells change monotonically and the few pairs that change cell
 * are found by the binary searches of mdb_hist_buckets.
 *   request: mdb_transit_request (mdb_format.h). buckets.t_lo / t_hi must be INT64_MIN / INT64_MAX and which_mask 0:
 *     the buckets are the range. reserved and flags must be 0, max_gap >= 0.
 *   edges, cells: those of mdb_hist_buckets - 1 .. MDB_HIST_MAX_EDGES edges, strictly increasing in totalOrder; the
 *     cell of a value is mdb_hist_cell_of; n_cells = n_edges + 1. A non-finite value is placed by its totalOrder key
 *     as in mdb_dwell_buckets: +NaN in the last cell, -NaN in the first, -0.0 below an edge at +0.0.
 *   counts: row-major uint64_t [n_groups][n_buckets][n_cells][n_cells], indexed [from][to]. A call ADDS to it.
 *   Rows and Linked: exactly those of mdb_integral_buckets - inside segments, across segments, across the inputs of
 *     the list form; not across calls. A segment that rebuilds to no row links nothing across it.
 *   The counter: mdb_change_buckets' rule. A linked pair (t0, v0) - (t1, v1) belongs to the bucket b of its LATER row
 *     and is never cut; it is dropped if t1 lies outside the buckets, t0 may lie anywhere. Each pair does
 *     counts[g][b][cell_of(v0)][cell_of(v1)] += 1.
 *   Finish: mdb_transit_crossings writes, per (group, bucket) row and edge e < n_edges, up[row][e] = the sum of
 *     counts[from <= e < to] and down[row][e] = the sum of counts[to <= e < from]: the pairs that went over edge e
 *     upwards and downwards. mdb_transit_merge_n adds two arrays.
 *   Exact promises: everything is a count, so every number is exact. (a) The n_cells^2 counters of a (group, bucket)
 *     row sum to mdb_change_buckets' count for the same request. (b) Adding the blocks of adjacent cells gives the
 *     matrix under the coarser edge list. (c) Adjacent buckets add up to the bucket of their union; moving the origin
 *     by whole widths, with n_buckets moved along, gives the same numbers. (d) The sum over `from` of
 *     counts[..][from][to] is the number of rows of the bucket in cell `to` that have a linked predecessor: for one
 *     fully linked series mdb_hist_buckets' count minus the first row. (e) Over buckets that cover one fully linked
 *     run, the sum over the buckets of up[e] - down[e] is (cell(last) > e) - (cell(first) > e). (f) The sum of
 *     counts[from > to] is at most mdb_change_buckets' n_fall.
 *   Determinism: integer atomics only; two runs and the three forms agree byte for byte, whatever the order of
 *     segments or the cut of batches at series boundaries.
 *   Errors (mdb_last_error set, counts untouched; what needs no device is checked before the device is used): a NULL
 *     argument, a bad edge list, width <= 0, n_groups == 0, n_groups * n_buckets * n_cells^2 overflowing or not
 *     fitting the device, a time range in the request, which_mask, reserved or flags != 0, a negative max_gap, a
 *     group id >= n_groups on ANY row, the malformed-segment classes of mdb_agg_buckets for the segments the request
 *     reaches and for the right neighbour whose first point a segment the request reaches may read (as
 *     mdb_change_buckets). An empty batch or n_buckets == 0 succeeds and changes nothing. */
int mdb_transit_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                        const mdb_transit_request *request, const float *edges, uint32_t n_edges, uint64_t *counts);
/* All device pointers but request and edges: the batch, group_of_segment and counts are in HBM. */
int mdb_transit_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                            const mdb_transit_request *request, const float *edges, uint32_t n_edges, uint64_t *counts);
/* Several host batches (rows in the order of the list) folded as one batch: a linked pair may cross from one input to
 * the next. group_of_segment: one array per batch, or NULL. */
int mdb_transit_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                             uint32_t n_inputs, const mdb_transit_request *request, const float *edges, uint32_t n_edges,
                             uint64_t *counts);
/* into[k] += from[k] for k < n. Host memory, no context. */
int mdb_transit_merge_n(uint64_t *into, const uint64_t *from, uint64_t n);
/* Per row < n_rows of n_cells * n_cells counters [from][to] and edge e < n_cells - 1: up[row * (n_cells - 1) + e] and
 * down[...] as above. n_cells must be at least 1 (1: nothing is written). Host memory, no context. */
int mdb_transit_crossings(const uint64_t *counts, uint64_t n_rows, uint32_t n_cells, uint64_t *up, uint64_t *down);

/* ---- fit: replaces try_compress_univariate_time_series
 *      (crates/modelardb_compression/src/compression.rs:191-275), called per field column by
 *      crates/modelardb_server/src/storage/uncompressed_data_manager.rs:563-581 and, through
 *      try_compress_multivariate_time_series (compression.rs:42-179), by
 *      crates/modelardb_embedded/src/operations/data_folder.rs:214-217 and
 *      crates/modelardb_bulkloader/src/main.rs:429-432 ------------------------------------------- */

/* Compress one sorted univariate series. n == 0 gives an empty batch (compression.rs:208-211). */
int mdb_compress_series(mdb_ctx *ctx, const int64_t *ts, const float *values, uint64_t n,
                        mdb_error_bound error_bound, mdb_segments_owned **out);

/* Compress many independent series chunks in one launch: chunk c is
 * [chunk_offsets[c], chunk_offsets[c + 1]) of ts/values. Segments come out grouped by chunk in
 * chunk order, each chunk's segments in time order; out->chunk_index names the chunk.
 * A BinaryView column whose payloads (irregular timestamps, MacaqueV values, residuals) add up to more
 * than 1 GiB comes back with several data buffers, as arrow's builders produce them (types.rs:444-516):
 * the views carry the buffer index, mdb_grid_* / mdb_agg_* read such columns, and mdb_segments_download
 * keeps the buffers apart when they do not fit into one. */
int mdb_compress_chunks(mdb_ctx *ctx, const int64_t *ts, const float *values,
                        const uint64_t *chunk_offsets, uint64_t n_chunks,
                        mdb_error_bound error_bound, mdb_segments_owned **out);

/* The same for chunks that lie wherever the caller has them (one slice of a sorted RecordBatch per series
 * and field, compression.rs:42-107; one finished ingest buffer per series and field,
 * uncompressed_data_manager.rs:530-596): the library gathers them into its page-locked staging block with
 * several threads while earlier parts cross PCIe, so the caller concatenates nothing. Chunks that share a
 * timestamp array (the fields of one series) are checked for regular spacing once. Output as above. */
int mdb_compress_chunk_list(mdb_ctx *ctx, const mdb_chunk *chunks, uint64_t n_chunks,
                            mdb_error_bound error_bound, mdb_segments_owned **out);

/* Device resident variant. ts may be NULL: then chunk c has the regular timestamps
 * regular_start + i * regular_interval (i counted from the start of the chunk's series, given by
 * series_first_index[c], or from 0 if that is NULL), synthesised on the fly. */
int mdb_compress_chunks_dev(mdb_ctx *ctx, const int64_t *ts, const float *values,
                            const uint64_t *chunk_offsets, uint64_t n_chunks,
                            mdb_error_bound error_bound, int64_t regular_start,
                            int64_t regular_interval, const uint64_t *series_first_index,
                            mdb_segments_owned **out);

/* try_split_and_compress_univariate_time_series (compression.rs:147-179): ONE sorted series with
 * n_fields field columns that share its timestamps, field f compressed within error_bounds[f].
 * out[f] receives field f's segments (host memory, as mdb_compress_series); on failure nothing is
 * returned. The timestamps cross PCIe once. */
int mdb_split_and_compress_univariate(mdb_ctx *ctx, const int64_t *ts, const float *const *field_values,
                                      const mdb_error_bound *error_bounds, uint32_t n_fields, uint64_t n,
                                      mdb_segments_owned **out);

/* ---- the crate's two remaining public helpers (crates/modelardb_compression/src/lib.rs:30-33):
 *      plain host arithmetic, no context, no GPU ------------------------------------------------- */

/* is_value_within_error_bound (models/mod.rs:53-77; used by tests of the callers, e.g.
 * crates/modelardb_server/tests/integration_test.rs:1232): *within = 1 or 0. */
int mdb_is_value_within_error_bound(mdb_error_bound error_bound, float real_value, float approximate_value,
                                    int32_t *within);
/* are_compressed_timestamps_regular (models/timestamps.rs:199-202; grid_exec.rs:352 feeds the
 * GridStreamMetrics with it): empty, or the top bit of the first byte is 0. */
int mdb_are_compressed_timestamps_regular(const uint8_t *compressed_timestamps, uint64_t n_bytes,
                                          int32_t *regular);

/* ---- multi-GPU: the final aggregate merge over RCCL / xGMI -----------------------
 * One process and one context per GPU; series are sharded over the GPUs and fit / grid / the
 * per-segment aggregates never exchange anything. The single exchange step is the merge of the
 * accumulators' partial states, which the reference hands to DataFusion's final aggregate
 * (crates/modelardb_storage/src/optimizer/model_simple_aggregates.rs:362-378, 517-534, 591-612). */

#define MDB_COMM_ID_BYTES 128
/* ncclGetUniqueId: called by ONE rank, which hands the 128 bytes to the others by whatever channel
 * the host has (the reference's cluster already talks Arrow Flight; the bench uses torch's store). */
int mdb_comm_unique_id(void *id_out);
/* ncclCommInitRank on the context's device; collective over all `world` ranks. */
int mdb_comm_init(mdb_ctx *ctx, int32_t rank, int32_t world, const void *unique_id);
int mdb_comm_close(mdb_ctx *ctx); /* also done by mdb_close */
/* Merge the partial states of all ranks: one ncclAllGather of 32 bytes per rank on the context's
 * stream, then a fold in RANK ORDER with the accumulators' own rules, so that the f64 SUM is
 * reproducible run to run and identical on every rank (an all-reduce leaves the order of the
 * additions to the ring). Collective. ranks_seen (may be NULL): how many states arrived. */
int mdb_agg_all_reduce(mdb_ctx *ctx, mdb_agg_state *inout, int32_t *ranks_seen);
/* The fold itself, for hosts that move the states themselves: into = merge(into, from). */
int mdb_agg_merge(mdb_agg_state *into, const mdb_agg_state *from);
/* The same for n states in a row: into[k] = merge(into[k], from[k]), k < n (host arithmetic, no context): the
 * fold of two cell arrays of mdb_agg_buckets* that a host has moved itself. n == 0 succeeds. */
int mdb_agg_merge_n(mdb_agg_state *into, const mdb_agg_state *from, uint64_t n);

/* ---- measurement ---------------------------------------------------------------------------- */

/* When enabled every kernel launch is bracketed with hipEvents on the context's stream. */
int mdb_profile_enable(mdb_ctx *ctx, int enabled);
int mdb_profile_reset(mdb_ctx *ctx);
/* Accumulated launches and milliseconds of kernel `name` since the last reset. mdb_compress_chunk_list adds the host
 * side of its calls under names that begin with "host:" (calls and wall-clock milliseconds): host:chunk_list_gather
 * (the host threads' copies into page-locked memory, the copies to the device running behind them),
 * host:chunk_list_upload_tail (what is left of those copies when the last slice is gathered), host:chunk_list_fit,
 * host:chunk_list_download. The jobs of mdb_grid_submit add theirs: host:grid_cursors_by_host_threads,
 * host:grid_wait_for_the_context, host:grid_upload_segments, host:grid_plan, host:grid_launches,
 * host:grid_kernels_and_copy_down, host:grid_free_segments. The profile of a context covers the clones its
 * mdb_grid_submit workers run jobs on: they are switched and reset with it, their launches are counted as its own. */
int mdb_profile_get(mdb_ctx *ctx, const char *name, uint64_t *launches, double *total_ms);
/* Names of all profiled kernels, '\n' separated. */
int mdb_profile_names(mdb_ctx *ctx, char *out, uint64_t cap);

/* Fill out[i] = synthetic series value: series s = first_series + i / n_per_series,
 * point j = i % n_per_series: 100 + 10 sin(2 pi j / P_s + phi_s) + U(-0.05, 0.05). Device buffer. */
int mdb_synth_values_dev(mdb_ctx *ctx, float *out, uint64_t first_series, uint64_t n_series,
                         uint64_t n_per_series, uint64_t seed);

#ifdef __cplusplus
}
#endif

#endif /* MDB_H */
