// mdb_hist.hip - value histograms and exact quantiles computed on segments (mdb_hist_batch*, mdb_quantile_batch*).
//
// What the reference computes with GridExec -> (FilterExec) -> AggregateExec for approx_percentile_cont / median /
// percentile_cont or a histogram of a field: its model-based rule (optimizer/model_simple_aggregates.rs) rewrites only
// COUNT / MIN / MAX / SUM / AVG, so a distribution rebuilds every point first (query/grid_exec.rs:366-387) and bins or
// sorts it afterwards. Here the points are counted per cell where they are, and never materialised:
//
//   k_hist_groups   every row's group id checked (also the rows the time range leaves out), before anything is counted.
//   k_hist          1 lane / segment that reaches into the time range, grid-strided and launched like k_agg_filter,
//                   with its analyse_segment, start / end rejection and error word. The edges' totalOrder keys sit in
//                   LDS (at most 16 KB, loaded once per workgroup). A lane keeps the key interval of its current cell
//                   and a pending run: a point is tested against that interval first (series are smooth) and only a
//                   miss costs a binary search of at most 12 steps over the LDS keys; a run goes to the cells with ONE
//                   64-bit integer atomic add. PMC-Mean on regular timestamps is one add of n; Swing is monotone in
//                   totalOrder (model_run, mdb_filter.hpp), so every edge it crosses is found by one binary search
//                   over the point index with exact evaluations (swing_first_past) - point by point instead when an
//                   end is NaN or when cells crossed * log2(n) would exceed n. Bit streams (MacaqueV values, residual
//                   tails, irregular timestamps) are decoded once by segment_range, unchanged, through the selector
//                   HistCells: its counts() records the point in the lane's run and selects nothing.
//   k_hist_fold     the scratch cells added into the caller's (the _dev form).
// The cells a pass counts into are zeroed scratch: the caller's counts are touched only after the pass has finished
// without an error - by k_hist_fold on the device, or on the host after one download. Integers only: the forms and
// any two runs agree bit for bit, and there is no float atomic.
// The quantiles are host code over the same pass (quantile_refine, mdb_hist.hpp): three passes of 4 096, 4 096 and 256
// cells pin an order statistic of the 32-bit keys exactly.
#include "mdb_hist.hpp"

#include "mdb_hist_dev.hpp"

#include <vector>

namespace mdb {

__global__ __launch_bounds__(HIST_THREADS) void k_hist_groups(const uint32_t *__restrict__ groups, uint64_t n,
                                                              uint32_t n_groups, unsigned int *__restrict__ error) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * HIST_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * HIST_THREADS)
        bad = bad || groups[i] >= n_groups;
    if (bad) atomicOr(error, ERR_HIST_GROUP);
}

// cells: n_groups rows of n_edges + 1 zeroed counters. (A row with a bad group id is skipped here as well: nothing is
// ever added outside the cells, whatever k_hist_groups has found.)
__global__ __launch_bounds__(HIST_THREADS) void k_hist(DevSegments s, const uint32_t *__restrict__ groups, int64_t t_lo,
                                                       int64_t t_hi, const int32_t *__restrict__ edge_keys,
                                                       uint32_t n_edges, uint32_t n_groups,
                                                       unsigned long long *__restrict__ cells,
                                                       unsigned int *__restrict__ error_word) {
    __shared__ int32_t lds_edges[MDB_HIST_MAX_EDGES + 1];
    for (uint32_t j = threadIdx.x; j < n_edges; j += HIST_THREADS) lds_edges[j] = edge_keys[j];
    __syncthreads();
    HistLane lane = {lds_edges, n_edges, cells, 1, 0, 0, 0};
    const uint64_t n_cells = (uint64_t)n_edges + 1;
    uint32_t errors = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * HIST_THREADS + threadIdx.x; i < s.n; i += (uint64_t)gridDim.x * HIST_THREADS) {
        if (s.end_time[i] < t_lo || s.start_time[i] > t_hi) continue;
        const uint32_t group = groups ? groups[i] : 0u;
        if (group >= n_groups) {
            errors |= ERR_HIST_GROUP;
            continue;
        }
        const SegInfo info = analyse_segment(s, i);
        uint32_t error = info.error;
        if (!error) {
            unsigned long long *row = cells + (uint64_t)group * n_cells;
            if (row != lane.cells) {
                lane.flush();
                lane.cells = row;
            }
            RangeAcc unused;
            segment_range(s, i, info, t_lo, t_hi, unused, &error, false, HistCells{&lane});
        }
        errors |= error;
    }
    lane.flush();
    if (errors) atomicOr(error_word, errors);
}

__global__ __launch_bounds__(HIST_THREADS) void k_hist_fold(const unsigned long long *__restrict__ cells, uint64_t n,
                                                            unsigned long long *__restrict__ counts) {
    for (uint64_t j = (uint64_t)blockIdx.x * HIST_THREADS + threadIdx.x; j < n; j += (uint64_t)gridDim.x * HIST_THREADS) {
        const unsigned long long added = cells[j];
        if (added) counts[j] += added;
    }
}

void hist_groups_launch(mdb_ctx *ctx, const uint32_t *groups, uint64_t n, uint32_t n_groups, unsigned int *error) {
    LaunchTimer timer(ctx, "k_hist_groups");
    hipLaunchKernelGGL(k_hist_groups, dim3(hist_blocks(n)), dim3(HIST_THREADS), 0, ctx->stream, groups, n, n_groups, error);
}

void hist_fold_launch(mdb_ctx *ctx, const unsigned long long *cells, uint64_t n, unsigned long long *counts) {
    LaunchTimer timer(ctx, "k_hist_fold");
    hipLaunchKernelGGL(k_hist_fold, dim3(hist_blocks(n)), dim3(HIST_THREADS), 0, ctx->stream, cells, n, counts);
}

namespace {

struct HistRequest { // a checked mdb_hist_request with its edges as keys
    int64_t t_lo, t_hi;
    uint32_t n_groups;
    std::vector<int32_t> edge_keys;
    uint64_t n_cells() const { return edge_keys.size() + 1; }
};

// The host-side checks every form makes before it touches the device.
int hist_request_check(const mdb_hist_request *request, const float *edges, HistRequest *out) {
    if (request->flags != 0 || request->reserved != 0) return fail("flags and reserved of the histogram request must be 0.");
    if (hist_edge_keys(edges, request->n_edges, &out->edge_keys)) return 1;
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    out->t_lo = request->t_lo;
    out->t_hi = request->t_hi;
    out->n_groups = request->n_groups;
    return 0;
}

// One pass: the points of the device batch `in` (groups: a device array or nullptr) inside the time range, counted
// into zeroed scratch cells and then ADDED to dev_counts (a device array) or host_counts (the caller's, after one
// download) - only once the pass is known to be free of errors.
int hist_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const HistRequest &r,
             unsigned long long *dev_counts, uint64_t *host_counts) {
    const uint64_t n = in->n;
    if (n == 0) return 0;
    const uint64_t total = (uint64_t)r.n_groups * r.n_cells(); // (below 2^44: no overflow)
    if (total * 8 > (1ull << 30)) { // (asked only where it could matter: more cells than the device has memory for)
        size_t free_bytes = 0, device_bytes = 0;
        MDB_HIP_CHECK(hipMemGetInfo(&free_bytes, &device_bytes));
        if (total * 8 > (uint64_t)device_bytes)
            return fail("n_groups * n_cells counters (" + std::to_string(total) + ") do not fit into the device's memory.");
    }
    void *p = nullptr;
    const uint64_t cells_bytes = align_up(total * 8, 256), keys_bytes = align_up(r.edge_keys.size() * 4, 256);
    if (scratch_reserve(ctx, SCRATCH_HIST_CELLS, cells_bytes + keys_bytes + 256, &p)) return 1;
    Carver scratch(p);
    unsigned long long *cells = scratch.take<unsigned long long>(total);
    int32_t *edge_keys = scratch.take<int32_t>(r.edge_keys.size());
    unsigned int *words = scratch.take<unsigned int>(2);
    MDB_HIP_CHECK(hipMemsetAsync(cells, 0, total * 8, ctx->stream));
    MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
    MDB_HIP_CHECK(mail_write(ctx, edge_keys, r.edge_keys.data(), r.edge_keys.size() * 4));
    if (groups) hist_groups_launch(ctx, groups, n, r.n_groups, words);
    {
        LaunchTimer timer(ctx, "k_hist");
        hipLaunchKernelGGL(k_hist, dim3(hist_blocks(n)), dim3(HIST_THREADS), 0, ctx->stream, to_dev(in), groups, r.t_lo,
                           r.t_hi, edge_keys, (uint32_t)r.edge_keys.size(), r.n_groups, cells, words);
    }
    unsigned int error = 0;
    MDB_HIP_CHECK(hipMemcpyAsync(&error, words, 4, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (error & ERR_HIST_GROUP) return fail("A group id is not below n_groups.");
    if (error) return fail(describe_error(error));
    if (host_counts) {
        std::vector<uint64_t> added(total);
        MDB_HIP_CHECK(hipMemcpyAsync(added.data(), cells, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (uint64_t j = 0; j < total; j++) host_counts[j] += added[j];
        return 0;
    }
    hist_fold_launch(ctx, cells, total, dev_counts);
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    return 0;
}

// The order statistics of the device batch `in`: quantile_refine over hist_run (one group, the counts to the host).
int quantile_run(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const double *q, uint32_t n_q,
                 float *out_lo, float *out_hi, uint64_t *n_points) {
    HistRequest r;
    r.t_lo = t_lo;
    r.t_hi = t_hi;
    r.n_groups = 1;
    return quantile_refine(
        q, n_q,
        [&](const float *edges, uint32_t n_edges, uint64_t *counts) {
            if (hist_edge_keys(edges, n_edges, &r.edge_keys)) return 1;
            return hist_run(ctx, in, nullptr, r, nullptr, counts);
        },
        out_lo, out_hi, n_points, nullptr);
}

} // namespace

} // namespace mdb

using namespace mdb;

extern "C" {

int mdb_hist_batch_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                       const mdb_hist_request *request, const float *edges, uint64_t *counts) {
    if (!ctx || !in || !request || !edges || !counts) return fail("ctx, in, request, edges and counts must not be NULL.");
    HistRequest r;
    if (hist_request_check(request, edges, &r)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return hist_run(ctx, in, group_of_segment, r, reinterpret_cast<unsigned long long *>(counts), nullptr);
}

int mdb_hist_batch_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                        uint32_t n_inputs, const mdb_hist_request *request, const float *edges, uint64_t *counts) {
    if (!ctx || !inputs || !request || !edges || !counts)
        return fail("ctx, inputs, request, edges and counts must not be NULL.");
    HistRequest r;
    if (hist_request_check(request, edges, &r)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0) return 0;
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, true)) return 1;
    return hist_run(ctx, list.segments(), list.groups(), r, nullptr, counts);
}

int mdb_hist_batch(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                   const mdb_hist_request *request, const float *edges, uint64_t *counts) {
    if (!in) return fail("ctx, in, request, edges and counts must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_hist_batch_list(ctx, &in, groups, 1, request, edges, counts);
}

int mdb_quantile_batch_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const double *q,
                           uint32_t n_q, float *out_lo, float *out_hi, uint64_t *n_points) {
    if (!ctx || !in || !q || !out_lo || !out_hi || !n_points)
        return fail("ctx, in, q, out_lo, out_hi and n_points must not be NULL.");
    if (quantile_arguments_check(q, n_q)) return 1;
    if (in->n == 0) { // (no point: the outputs stay as they are)
        *n_points = 0;
        return 0;
    }
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return quantile_run(ctx, in, t_lo, t_hi, q, n_q, out_lo, out_hi, n_points);
}

int mdb_quantile_batch(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const double *q, uint32_t n_q,
                       float *out_lo, float *out_hi, uint64_t *n_points) {
    if (!ctx || !in || !q || !out_lo || !out_hi || !n_points)
        return fail("ctx, in, q, out_lo, out_hi and n_points must not be NULL.");
    if (quantile_arguments_check(q, n_q)) return 1;
    if (in->n == 0) { // (no point: the outputs stay as they are)
        *n_points = 0;
        return 0;
    }
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    // (uploaded once: every pass of the refinement reads the resident copy)
    mdb_segments_owned *dev = nullptr;
    if (upload_segments_locked(ctx, in, true, &dev)) return 1;
    const int rc = quantile_run(ctx, &dev->seg, t_lo, t_hi, q, n_q, out_lo, out_hi, n_points);
    mdb_segments_free(dev);
    return rc;
}

int mdb_hist_cell_of(const float *edges, uint32_t n_edges, float value, uint32_t *cell) {
    if (!edges || !cell) return fail("edges and cell must not be NULL.");
    std::vector<int32_t> keys;
    if (hist_edge_keys(edges, n_edges, &keys)) return 1;
    *cell = hist_cell_of_key(keys, hist_key_of(value));
    return 0;
}

int mdb_quantile_positions(double q, uint64_t n_points, uint64_t *rank_lo, uint64_t *rank_hi, double *fraction) {
    if (!rank_lo || !rank_hi || !fraction) return fail("rank_lo, rank_hi and fraction must not be NULL.");
    uint64_t lo = 0, hi = 0;
    double part = 0.0;
    if (quantile_ranks(q, n_points, &lo, &hi, &part)) return 1;
    *rank_lo = lo;
    *rank_hi = hi;
    *fraction = part;
    return 0;
}

} // extern "C"
