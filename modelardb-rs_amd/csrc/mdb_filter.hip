// mdb_filter.hip - a value predicate pushed down to the segments (mdb_grid_*_filter*, mdb_agg_batch_filter*).
//
// What the reference computes with GridExec -> FilterExec (and -> AggregateExec) for WHERE field op literal
// [AND ts ...]: query/time_series_table.rs:290-370 rewrites only the predicates on the timestamp, so the one on the
// value stays in a FilterExec above GridExec, which rebuilds every point first (query/grid_exec.rs:366-387). Here the
// predicate (mdb_value_filter, IEEE totalOrder on the f32 bits, folded once on the host into a closed interval of
// integer keys, mdb_filter.hpp) is applied on the segments:
//
//   k_filter_classify    1 lane / segment, after the range grid's own prepass (grid_range_plan: the segment
//                        counters of the metrics, and every error the range calls report). Each time-clipped segment
//                        goes into one of three classes: none (PMC-Mean whose value fails; Swing whose evaluated
//                        ends fail on the same side), one interval [a, b] of model points (PMC-Mean whose value
//                        passes; the model part of Swing on regular timestamps, two binary searches over k -
//                        model_run), or per point (MacaqueV, irregular timestamps, a Swing end that is NaN). A
//                        residual tail is per point on its own; its segment's model part is classified as above.
//   per-point segments   gathered into a batch of their own (k_filter_gather: the columns, with the same payload
//                        buffers) and rebuilt by the range grid itself (grid_batch_dev_locked) in slices of at most
//                        MDB_FILTER_SLICE_POINTS points (less under mdb_set_scratch_limit; filter_tested_slices);
//                        k_filter_points_count / k_filter_points_write then compact each segment's rows with one wave
//                        (slice_walk, mdb_filter_points.hpp: the walk the row masks' k_mask_points_* share): __ballot
//                        of the predicate, a prefix from __popcll, stable. Such segments are rebuilt twice (once to
//                        count, once to write) unless all of them fit into one slice, which is then kept between the
//                        passes.
//   scan                 rows per segment -> 64-bit output offsets (mdb_scan.hpp); one read-back sizes the output.
//   k_filter_write_runs  1 wave / interval segment: start + k * delta and its model value for k in [a, b].
// Rows come out in segment order and point order, exactly mdb_grid_batch_range's rows minus the ones that fail.
// Also here, for the row masks (mdb_mask.hip) and the plain grid (mdb_grid.hip) too: what a count leaves for its write
// (filter_count_done) and the result block of the owned forms (result_layout, owned_block_copy, owned_result_make).
// All writes are ordinary vector stores; the only atomics are integer ones on LDS and on the three row counters.
//
// The filtered aggregates are k_agg_range's loop with the predicate (mdb_agg.hip, k_agg_filter): segment_range's
// closed forms over the interval of a PMC-Mean / Swing model part, a test per point in its decoders.
#include "mdb_agg_dev.hpp"
#include "mdb_filter.hpp"
#include "mdb_filter_points.hpp"
#include "mdb_host_side.hpp"
#include "mdb_scan.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace mdb {

constexpr uint64_t FILTER_SLICE_DEFAULT = 1ull << 24; // points per slice of the per-point segments: 192 MB of rows

// (FilterRun, classify_segment, Gathered, FilterPass: mdb_filter_points.hpp - shared with the row masks)

// counts[i]: the passing model points of segment i's interval (its final row count once k_filter_points_count has added
// the per-point ones). per_point[i]: 0 - no point of segment i is tested one by one; 1 + m - its rows in the range
// grid are tested from the (m + 1)-th on (m: the model rows the interval has already decided).
__global__ __launch_bounds__(FILTER_THREADS) void k_filter_classify(DevSegments s, int64_t t_lo, int64_t t_hi,
                                                                    ValueKeys keys, FilterRun *__restrict__ runs,
                                                                    uint32_t *__restrict__ counts,
                                                                    uint32_t *__restrict__ per_point) {
    const uint64_t i = (uint64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
    if (i >= s.n) return;
    FilterRun r;
    uint32_t tested = 0, run_first = 0;
    classify_segment(s, i, t_lo, t_hi, keys, &r, &tested, &run_first);
    runs[i] = r;
    counts[i] = r.n;
    per_point[i] = tested;
}

struct FilterTested { // (scan functor: the segments with points tested one by one)
    const uint32_t *per_point;
    __device__ uint64_t operator()(uint64_t i) const { return per_point[i] != 0 ? 1u : 0u; }
};

__global__ __launch_bounds__(FILTER_THREADS) void k_filter_gather(DevSegments s, const uint32_t *__restrict__ per_point,
                                                                  const unsigned long long *__restrict__ position,
                                                                  Gathered g) {
    const uint64_t i = (uint64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
    if (i >= s.n || per_point[i] == 0) return;
    const uint64_t j = position[i];
    g.type[j] = s.model_type_id[i];
    g.start[j] = s.start_time[i];
    g.end[j] = s.end_time[i];
    g.min[j] = s.min_value[i];
    g.max[j] = s.max_value[i];
    g.ts_views[j] = s.timestamps.views[i];
    g.value_views[j] = s.values.views[i];
    g.residual_views[j] = s.residuals.views[i];
    g.origin[j] = (uint32_t)i;
    g.skip[j] = per_point[i] - 1;
}

// The per-point segments of a slice (slice_walk, mdb_filter_points.hpp), their rows tested by value: the passing ones
// added to counts[origin] ...
__global__ __launch_bounds__(FILTER_THREADS) void k_filter_points_count(const float *__restrict__ slice_val,
                                                                        const unsigned long long *__restrict__ first,
                                                                        uint64_t n_slice, uint64_t j0, Gathered g,
                                                                        ValueKeys keys, uint32_t *__restrict__ counts) {
    slice_walk(first, n_slice, j0, g, [&](uint32_t, uint64_t) { return [&](uint64_t row) { return keys.pass(slice_val[row]); }; },
               [](uint32_t, uint64_t) { return [](uint64_t, uint64_t, bool, unsigned long long, uint64_t) {}; },
               [&](uint32_t origin, uint64_t kept) {
                   if ((threadIdx.x & (MDB_WAVE - 1)) == 0) counts[origin] += (uint32_t)kept;
               });
}
// ... or written, in order, behind the segment's interval rows.
__global__ __launch_bounds__(FILTER_THREADS) void k_filter_points_write(
    const int64_t *__restrict__ slice_ts, const float *__restrict__ slice_val, const unsigned long long *__restrict__ first,
    uint64_t n_slice, uint64_t j0, Gathered g, ValueKeys keys, const FilterRun *__restrict__ runs,
    const unsigned long long *__restrict__ offsets, int64_t *__restrict__ out_ts, float *__restrict__ out_val) {
    slice_walk(first, n_slice, j0, g, [&](uint32_t, uint64_t) { return [&](uint64_t row) { return keys.pass(slice_val[row]); }; },
               [&](uint32_t origin, uint64_t) {
                   const uint64_t out = offsets[origin] + runs[origin].n;
                   return [&, out](uint64_t, uint64_t row, bool pass, unsigned long long ballot, uint64_t kept) {
                       slice_write_row(out + kept, row, pass, ballot, slice_ts, slice_val, out_ts, out_val);
                   };
               },
               [](uint32_t, uint64_t) {});
}

// One wave per interval segment: its n points from offsets[i] on.
__global__ __launch_bounds__(FILTER_THREADS) void k_filter_write_runs(const FilterRun *__restrict__ runs, uint64_t n,
                                                                      const unsigned long long *__restrict__ offsets,
                                                                      int64_t *__restrict__ out_ts,
                                                                      float *__restrict__ out_val) {
    const uint32_t lane = threadIdx.x & (MDB_WAVE - 1);
    const uint64_t waves = (uint64_t)gridDim.x * (FILTER_THREADS / MDB_WAVE);
    for (uint64_t i = (uint64_t)blockIdx.x * (FILTER_THREADS / MDB_WAVE) + threadIdx.x / MDB_WAVE; i < n; i += waves) {
        const FilterRun r = runs[i];
        if (r.n == 0) continue;
        const uint64_t base = offsets[i];
        for (uint32_t k = lane; k < r.n; k += MDB_WAVE) {
            int64_t t;
            float v;
            run_point(r, k, &t, &v);
            out_ts[base + k] = t;
            out_val[base + k] = v;
        }
    }
}

// rows_created_by_model_type of the rows produced: per block in LDS, then one integer atomic per block and type.
__global__ __launch_bounds__(FILTER_THREADS) void k_filter_rows_by_type(const int8_t *__restrict__ types,
                                                                        const uint32_t *__restrict__ counts, uint64_t n,
                                                                        unsigned long long *__restrict__ by_type) {
    __shared__ unsigned long long lds[3];
    if (threadIdx.x < 3) lds[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long local[3] = {0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * FILTER_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FILTER_THREADS) {
        const int type = types[i];
        if (type >= 0 && type < 3) local[type] += counts[i];
    }
    for (int k = 0; k < 3; k++)
        if (local[k]) atomicAdd(&lds[k], local[k]);
    __syncthreads();
    if (threadIdx.x < 3 && lds[threadIdx.x]) atomicAdd(&by_type[threadIdx.x], lds[threadIdx.x]);
}

namespace {

// MDB_FILTER_SLICE_POINTS: points of the per-point segments rebuilt at once (bounded scratch); under
// mdb_set_scratch_limit at most a quarter of the limit's worth of rows (12 B each).
uint64_t slice_points(const mdb_ctx *ctx) {
    uint64_t points = FILTER_SLICE_DEFAULT;
    if (const char *text = option_text("MDB_FILTER_SLICE_POINTS")) {
        const long long value = std::atoll(text);
        if (value >= 1) points = (uint64_t)value;
    }
    if (ctx->scratch_limit) points = std::min<uint64_t>(points, std::max<uint64_t>(ctx->scratch_limit / 48, 1024));
    return points;
}

} // namespace

// The range grid of gathered segments [j0, j1) into the slice buffers, and the first row of each.
int filter_rebuild_slice(mdb_ctx *ctx, FilterPass &f, uint64_t j0, uint64_t j1) {
    mdb_segments part = f.tested;
    part.n = j1 - j0;
    part.model_type_id = f.tested.model_type_id + j0;
    part.start_time = f.tested.start_time + j0;
    part.end_time = f.tested.end_time + j0;
    part.min_value = f.tested.min_value + j0;
    part.max_value = f.tested.max_value + j0;
    part.timestamps.views = f.tested.timestamps.views + j0;
    part.values.views = f.tested.values.views + j0;
    part.residuals.views = f.tested.residuals.views + j0;
    uint64_t produced = 0;
    if (grid_batch_dev_locked(ctx, &part, TimeRange{f.t_lo, f.t_hi, 1}, f.slice_ts, f.slice_val, f.slice_rows,
                              f.slice_cap, &produced, nullptr))
        return 1;
    return device_exclusive_scan(ctx, ItemsOf<uint32_t>{f.slice_rows}, part.n, f.slice_first, f.slice_block_sums,
                                 "k_filter_scan");
}

// The per-point segments of f.in (per_point[i] != 0) gathered, their slices planned, the slice buffers reserved.
int filter_gather_tested(mdb_ctx *ctx, FilterPass &f, const uint32_t *per_point, unsigned long long *position,
                         unsigned long long *block_sums) {
    const mdb_segments *in = f.in;
    const uint64_t n = in->n;
    const DevSegments s = to_dev(in);
    const uint32_t blocks = (uint32_t)((n + FILTER_THREADS - 1) / FILTER_THREADS);
    void *p = nullptr;
    if (device_exclusive_scan(ctx, FilterTested{per_point}, n, position, block_sums, "k_filter_scan")) return 1;
    MDB_HIP_CHECK(hipMemcpyAsync(&f.n_tested, position + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (f.n_tested == 0) return 0;
    {
        const uint64_t m = f.n_tested;
        const uint64_t b8 = align_up(m * 8, 256), b4 = align_up(m * 4, 256), b16 = align_up(m * 16, 256), b1 = align_up(m, 256);
        if (scratch_reserve(ctx, SCRATCH_FILTER_GATHER, b1 + 2 * b8 + 5 * b4 + 3 * b16, &p)) return 1;
        Carver gathered(p);
        f.g.start = gathered.take<int64_t>(m);
        f.g.end = gathered.take<int64_t>(m);
        f.g.ts_views = gathered.take<uint4>(m);
        f.g.value_views = gathered.take<uint4>(m);
        f.g.residual_views = gathered.take<uint4>(m);
        f.g.min = gathered.take<float>(m);
        f.g.max = gathered.take<float>(m);
        f.g.origin = gathered.take<uint32_t>(m);
        f.g.skip = gathered.take<uint32_t>(m);
        f.g.rows = gathered.take<uint32_t>(m);
        f.g.type = gathered.take<int8_t>(m);
        {
            LaunchTimer timer(ctx, "k_filter_gather");
            hipLaunchKernelGGL(k_filter_gather, dim3(blocks), dim3(FILTER_THREADS), 0, ctx->stream, s, per_point, position,
                               f.g);
        }
        f.tested = *in;
        f.tested.n = m;
        f.tested.model_type_id = f.g.type;
        f.tested.start_time = f.g.start;
        f.tested.end_time = f.g.end;
        f.tested.min_value = f.g.min;
        f.tested.max_value = f.g.max;
        f.tested.timestamps.views = reinterpret_cast<const mdb_view16 *>(f.g.ts_views);
        f.tested.values.views = reinterpret_cast<const mdb_view16 *>(f.g.value_views);
        f.tested.residuals.views = reinterpret_cast<const mdb_view16 *>(f.g.residual_views);
        // Their rows in the range grid, and slices of at most slice_points() of them (one segment at least).
        uint64_t tested_rows = 0;
        if (grid_range_plan(ctx, &f.tested, f.t_lo, f.t_hi, &tested_rows, nullptr, f.g.rows)) return 1;
        const uint64_t budget = slice_points(ctx);
        if (tested_rows <= budget) {
            f.slices.push_back({0, m});
            f.slice_cap = tested_rows;
        } else {
            std::vector<uint32_t> rows(m);
            MDB_HIP_CHECK(hipMemcpyAsync(rows.data(), f.g.rows, m * 4, hipMemcpyDeviceToHost, ctx->stream));
            MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            uint64_t j0 = 0, held = 0;
            for (uint64_t j = 0; j < m; j++) {
                if (j > j0 && held + rows[j] > budget) {
                    f.slices.push_back({j0, j});
                    f.slice_cap = std::max(f.slice_cap, held);
                    j0 = j;
                    held = 0;
                }
                held += rows[j];
            }
            f.slices.push_back({j0, m});
            f.slice_cap = std::max(f.slice_cap, held);
        }
        const uint64_t cap = std::max<uint64_t>(f.slice_cap, 1);
        const uint64_t sts = align_up(cap * 8, 256), sval = align_up(cap * 4, 256);
        const uint64_t srows = align_up(m * 4, 256), sfirst = align_up((m + 1) * 8, 256);
        if (scratch_reserve(ctx, SCRATCH_FILTER_SLICE, sts + sval + srows + sfirst + align_up(scan_block_sums_bytes(m), 256), &p))
            return 1;
        Carver slice(p);
        f.slice_ts = slice.take<int64_t>(cap);
        f.slice_val = slice.take<float>(cap);
        f.slice_rows = slice.take<uint32_t>(m);
        f.slice_first = slice.take<unsigned long long>(m + 1);
        f.slice_block_sums = slice.take<unsigned long long>(scan_block_sums_bytes(m) / 8);
    }
    return 0;
}

// by_type[k] (three words in HBM) = the sum of counts[i] over the segments of model type k.
static int filter_rows_by_type(mdb_ctx *ctx, const int8_t *types, const uint32_t *counts, uint64_t n,
                               unsigned long long *by_type) {
    MDB_HIP_CHECK(hipMemsetAsync(by_type, 0, 3 * 8, ctx->stream));
    if (n == 0) return 0;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + FILTER_THREADS - 1) / FILTER_THREADS, 1024);
    LaunchTimer timer(ctx, "k_filter_rows_by_type");
    hipLaunchKernelGGL(k_filter_rows_by_type, dim3(blocks), dim3(FILTER_THREADS), 0, ctx->stream, types, counts, n, by_type);
    return 0;
}

int filter_count_done(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *counts, unsigned long long *offsets,
                      unsigned long long *block_sums, unsigned long long *by_type, const char *scan_name, uint64_t *total,
                      mdb_grid_metrics *metrics) {
    const uint64_t n = in->n;
    if (device_exclusive_scan(ctx, ItemsOf<uint32_t>{counts}, n, offsets, block_sums, scan_name)) return 1;
    if (filter_rows_by_type(ctx, in->model_type_id, counts, n, by_type)) return 1;
    unsigned long long words[4] = {0, 0, 0, 0};
    MDB_HIP_CHECK(hipMemcpyAsync(&words[0], offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipMemcpyAsync(&words[1], by_type, 3 * 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    *total = words[0];
    metrics->rows_created = words[0];
    for (int k = 0; k < 3; k++) metrics->rows_created_by_model_type[k] = words[1 + k];
    return 0;
}

ResultLayout result_layout(uint64_t reserve_front, uint64_t n, uint64_t n_segments, bool values_only) {
    const uint64_t front = align_up(reserve_front, 4); // keeps the 16-byte store alignment
    return ResultLayout{front, n, n_segments, values_only ? 0 : align_up((front + n) * 8, 256), align_up((front + n) * 4, 256),
                        align_up(n_segments * 4, 256), values_only};
}

int owned_block_copy(mdb_ctx *ctx, const void *stage, const ResultLayout &layout, void **block, uint64_t *capacity) {
    if (ctx->pinned_pool->take(layout.bytes(), block, capacity)) return 1;
    if (!stage) {
        std::memset(layout.rows(*block), 0, layout.rows_bytes);
    } else if (hipMemcpyAsync(*block, stage, layout.bytes(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
        ctx->pinned_pool->give(*block, *capacity);
        return fail("hipMemcpy device to host failed.");
    }
    return 0;
}

int owned_result_make(mdb_ctx *ctx, int rc, const ResultLayout &layout, void *block, uint64_t capacity,
                      const mdb_grid_metrics &metrics, mdb_grid_result **out) {
    if (rc) {
        ctx->pinned_pool->give(block, capacity);
        return rc;
    }
    OwnedGridResult *result = new OwnedGridResult();
    result->c.timestamps = layout.timestamps(block);
    result->c.values = layout.values(block);
    result->c.rows_per_segment = layout.rows(block);
    result->c.n = layout.n;
    result->c.n_segments = layout.n_segments;
    result->c.reserved_front = layout.front;
    result->c.metrics = metrics;
    result->c.priv_ = result;
    result->pool = ctx->pinned_pool;
    result->block = block;
    result->capacity = capacity;
    *out = &result->c;
    return 0;
}

int owned_result(mdb_ctx *ctx, const void *stage, const ResultLayout &layout, const mdb_grid_metrics &metrics,
                 mdb_grid_result **out) {
    void *block = nullptr;
    uint64_t capacity = 0;
    if (owned_block_copy(ctx, stage, layout, &block, &capacity)) return 1;
    const int rc = stage && hipStreamSynchronize(ctx->stream) != hipSuccess ? fail("hipMemcpy device to host failed.") : 0;
    return owned_result_make(ctx, rc, layout, block, capacity, metrics, out);
}

namespace {

// Pass 1: classify, count the per-point segments' passing rows (slice by slice), scan. Sets f.total and f.metrics.
int filter_count(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, FilterPass &f) {
    f.in = in;
    f.t_lo = filter->t_lo;
    f.t_hi = filter->t_hi;
    if (value_keys_fold(filter, &f.keys)) return 1;
    // The range grid's prepass: its segment counters and its verdict on the segments.
    uint64_t range_total = 0;
    if (grid_range_plan(ctx, in, f.t_lo, f.t_hi, &range_total, &f.metrics, nullptr)) return 1;
    const uint64_t n = in->n;
    if (n == 0) return 0;
    if (n > 0xffffffffull) return fail("Too many segments for one filtered call.");
    const DevSegments s = to_dev(in);
    const uint64_t runs_bytes = align_up(n * sizeof(FilterRun), 256), words_bytes = align_up(n * 4, 256);
    const uint64_t offsets_bytes = align_up((n + 1) * 8, 256), sums_bytes = align_up(scan_block_sums_bytes(n), 256);
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_FILTER_SEGMENTS, runs_bytes + 2 * words_bytes + 2 * offsets_bytes + sums_bytes + 256, &p))
        return 1;
    Carver segments(p);
    f.runs = segments.take<FilterRun>(n);
    f.counts = segments.take<uint32_t>(n);
    uint32_t *per_point = segments.take<uint32_t>(n);
    f.offsets = segments.take<unsigned long long>(n + 1);
    unsigned long long *position = segments.take<unsigned long long>(n + 1);
    unsigned long long *block_sums = segments.take<unsigned long long>(scan_block_sums_bytes(n) / 8);
    unsigned long long *by_type = segments.take<unsigned long long>(3);
    const uint32_t blocks = (uint32_t)((n + FILTER_THREADS - 1) / FILTER_THREADS);
    {
        LaunchTimer timer(ctx, "k_filter_classify");
        hipLaunchKernelGGL(k_filter_classify, dim3(blocks), dim3(FILTER_THREADS), 0, ctx->stream, s, f.t_lo, f.t_hi,
                           f.keys, f.runs, f.counts, per_point);
    }
    if (filter_tested_slices(ctx, f, per_point, position, block_sums, [&](uint64_t j0, uint64_t n_slice) {
            LaunchTimer timer(ctx, "k_filter_points_count");
            hipLaunchKernelGGL(k_filter_points_count, dim3(slice_walk_blocks(n_slice, 8192)), dim3(FILTER_THREADS), 0,
                               ctx->stream, f.slice_val, f.slice_first, n_slice, j0, f.g, f.keys, f.counts);
        }))
        return 1;
    return filter_count_done(ctx, in, f.counts, f.offsets, block_sums, by_type, "k_filter_scan", &f.total, &f.metrics);
}

// Pass 2: the rows into out_ts / out_val (f.total of them), rows per segment into out_rows (may be nullptr).
int filter_write(mdb_ctx *ctx, FilterPass &f, int64_t *out_ts, float *out_val, uint32_t *out_rows) {
    const uint64_t n = f.in->n;
    if (n == 0) return 0;
    if (f.total > 0) {
        {
            LaunchTimer timer(ctx, "k_filter_write_runs");
            hipLaunchKernelGGL(k_filter_write_runs, dim3(slice_walk_blocks(n, 16384)), dim3(FILTER_THREADS), 0, ctx->stream,
                               f.runs, n, f.offsets, out_ts, out_val);
        }
        if (filter_tested_slices(ctx, f, nullptr, nullptr, nullptr, [&](uint64_t j0, uint64_t n_slice) {
                LaunchTimer timer(ctx, "k_filter_points_write");
                hipLaunchKernelGGL(k_filter_points_write, dim3(slice_walk_blocks(n_slice, 8192)), dim3(FILTER_THREADS), 0,
                                   ctx->stream, f.slice_ts, f.slice_val, f.slice_first, n_slice, j0, f.g, f.keys, f.runs,
                                   f.offsets, out_ts, out_val);
            }))
            return 1;
    }
    if (out_rows) MDB_HIP_CHECK(hipMemcpyAsync(out_rows, f.counts, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int grid_count_filter_locked(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, uint64_t *n_out) {
    FilterPass f;
    if (filter_count(ctx, in, filter, f)) return 1;
    *n_out = f.total;
    return 0;
}

int grid_batch_filter_locked(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, int64_t *out_ts,
                             float *out_val, uint32_t *out_rows, uint64_t cap, uint64_t *n_out,
                             mdb_grid_metrics *metrics) {
    FilterPass f;
    if (filter_count(ctx, in, filter, f)) return 1;
    if (f.total > cap)
        return fail("Output buffers too small: " + std::to_string(f.total) + " data points but capacity " +
                    std::to_string(cap) + ".");
    if (f.total > 0 && (!out_ts || !out_val)) return fail("out_ts and out_val must not be NULL.");
    if (filter_write(ctx, f, out_ts, out_val, out_rows)) return 1;
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (n_out) *n_out = f.total;
    if (metrics) *metrics = f.metrics;
    return 0;
}

} // namespace

} // namespace mdb

using namespace mdb;

extern "C" {

int mdb_grid_count_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, uint64_t *n_out) {
    if (!ctx || !in || !filter || !n_out) return fail("ctx, in, filter and n_out must not be NULL.");
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return grid_count_filter_locked(ctx, in, filter, n_out);
}

int mdb_grid_batch_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, int64_t *out_ts,
                              float *out_val, uint32_t *out_rows_per_segment, uint64_t cap, uint64_t *n_out,
                              mdb_grid_metrics *metrics) {
    if (!ctx || !in || !filter) return fail("ctx, in and filter must not be NULL.");
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return grid_batch_filter_locked(ctx, in, filter, out_ts, out_val, out_rows_per_segment, cap, n_out, metrics);
}

int mdb_grid_batch_filter_owned(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter,
                                uint64_t reserve_front, mdb_grid_result **out) {
    if (!ctx || !in || !filter || !out) return fail("ctx, in, filter and out must not be NULL.");
    ValueKeys keys;
    if (value_keys_fold(filter, &keys)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    mdb_segments_owned *dev = nullptr;
    if (upload_segments_locked(ctx, in, true, &dev)) return 1;
    FilterPass f;
    int rc = filter_count(ctx, &dev->seg, filter, f);
    const ResultLayout layout = result_layout(reserve_front, f.total, dev->seg.n, false);
    void *stage = nullptr;
    if (!rc) rc = scratch_reserve(ctx, SCRATCH_STAGE_DEV, layout.bytes(), &stage);
    if (!rc) rc = filter_write(ctx, f, layout.timestamps(stage), layout.values(stage), layout.rows(stage));
    if (!rc) rc = owned_result(ctx, stage, layout, f.metrics, out);
    mdb_segments_free(dev);
    return rc;
}

int mdb_agg_batch_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, uint32_t which_mask,
                             mdb_agg_state *inout) {
    if (!ctx || !in || !filter || !inout) return fail("ctx, in, filter and inout must not be NULL.");
    ValueKeys keys;
    if (value_keys_fold(filter, &keys)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return agg_filter_run(ctx, in, filter->t_lo, filter->t_hi, keys, which_mask, inout);
}

int mdb_agg_batch_filter(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, uint32_t which_mask,
                         mdb_agg_state *inout) {
    if (!in) return fail("ctx, in, filter and inout must not be NULL.");
    return mdb_agg_batch_filter_list(ctx, &in, 1, filter, which_mask, inout);
}

int mdb_agg_batch_filter_list(mdb_ctx *ctx, const mdb_segments *const *inputs, uint32_t n_inputs,
                              const mdb_value_filter *filter, uint32_t which_mask, mdb_agg_state *inout) {
    if (!ctx || !inputs || !filter || !inout) return fail("ctx, inputs, filter and inout must not be NULL.");
    for (uint32_t k = 0; k < n_inputs; k++)
        if (!inputs[k]) return fail("A batch of the list is NULL.");
    ValueKeys keys;
    if (value_keys_fold(filter, &keys)) return 1;
    if (n_inputs == 0) return 0;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    mdb_segments_owned *dev = nullptr;
    if (upload_segment_list_locked(ctx, inputs, n_inputs, true, &dev)) return 1;
    const int rc = agg_filter_run(ctx, &dev->seg, filter->t_lo, filter->t_hi, keys, which_mask, inout);
    mdb_segments_free(dev);
    return rc;
}

} // extern "C"
