// mdb_transit.hip - transitions between value cells per date_bin bucket and group, computed on segments
// (mdb_transit_buckets*): counts[group][bucket][from][to], the linked pairs of rows whose later row lies in the bucket,
// by the cells of their two values, in one pass over the batch.
//
// What the reference can only answer with GridExec -> WindowAggExec(lag) -> AggregateExec GROUP BY date_bin,
// width_bucket(lag), width_bucket over every rebuilt point. Here a (segment, bucket) pair is one add for PMC-Mean, and
// for Swing on regular timestamps one add per cell its line passes and one per edge it crosses, found by the binary
// searches of k_hist_buckets. k_dwell_buckets' shape with k_change_partials' pairs:
//
//   k_hist_groups      (mdb_hist.hip) every row's group id checked, also the rows the request leaves out.
//   k_transit_heads    1 lane / segment whose left neighbour shares its group and reaches a bucket: its rows and the
//                      value of its first row (integral_head_of), 8 B / segment. k_integral_heads without the pair
//                      offsets, which this operator has no other use for: the left neighbour's span is computed
//                      instead of read, and the scan that makes the offsets is not run.
//   k_transit_buckets  1 lane / segment, grid-strided and launched like k_hist_buckets, the edges' keys in LDS. The
//                      lane's buckets are those its extent [start_time, linked ? start_time of the next : end_time]
//                      overlaps (integral_span): the pair with the right neighbour's first row belongs to the left
//                      segment. What a lane makes of its segment is mdb_transit.hpp's transit_segment; its run is
//                      flushed wherever the counter changes.
//   k_hist_fold        (mdb_hist.hip) the scratch counters added into the caller's (the _dev form).
// Integers only, integer atomics on zeroed scratch counters, which are added to the caller's array only once the
// error word has been read back clean: the forms and any two runs agree bit for bit. Every stream is one lane's: the
// batch's cursor index is not used (as k_hist_buckets).
//
// Scratch: 8 B per counter, the edges' keys and the error word (SCRATCH_HIST_CELLS); 8 B per segment of heads
// (SCRATCH_INTEGRAL_HEADS).
#include "mdb_transit.hpp"

#include <vector>

namespace mdb {

__global__ __launch_bounds__(HIST_THREADS) void k_transit_heads(DevSegments s, const uint32_t *__restrict__ groups,
                                                                IntegralRequest q, IntegralHead *__restrict__ heads,
                                                                unsigned int *__restrict__ error_word) {
    const uint64_t i = (uint64_t)blockIdx.x * HIST_THREADS + threadIdx.x;
    if (i == 0 || i >= s.n) return;
    uint64_t first = 0;
    if (!integral_same_group(groups, i - 1, i) || integral_span(s, groups, i - 1, q, &first) == 0) return; // (never read)
    const SegInfo info = analyse_segment(s, i);
    uint32_t error = info.error;
    heads[i] = error ? IntegralHead{0.0f, info.desc.n_total} : integral_head_of(s, i, info, &error);
    if (error) atomicOr(error_word, error);
}

// cells: n_groups * n_buckets matrices of (n_edges + 1)^2 zeroed counters. (A row with a bad group id is skipped here
// as well: nothing is ever added outside the cells, whatever k_hist_groups has found.)
__global__ __launch_bounds__(HIST_THREADS) void k_transit_buckets(DevSegments s, const uint32_t *__restrict__ groups,
                                                                  IntegralRequest q, const int32_t *__restrict__ edge_keys,
                                                                  uint32_t n_edges, const IntegralHead *__restrict__ heads,
                                                                  unsigned long long *__restrict__ cells,
                                                                  unsigned int *__restrict__ error_word) {
    __shared__ int32_t lds_keys[MDB_HIST_MAX_EDGES + 1];
    for (uint32_t j = threadIdx.x; j < n_edges; j += HIST_THREADS) lds_keys[j] = edge_keys[j];
    __syncthreads();
    TransitLane lane = {lds_keys, n_edges, nullptr, 0, 1, 0, 0};
    uint32_t errors = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * HIST_THREADS + threadIdx.x; i < s.n; i += (uint64_t)gridDim.x * HIST_THREADS) {
        uint64_t b_first = 0;
        const uint64_t count = integral_span(s, groups, i, q, &b_first);
        if (count == 0) continue;
        const uint32_t group = groups ? groups[i] : 0u;
        if (group >= q.buckets.n_groups) {
            errors |= ERR_HIST_GROUP;
            continue;
        }
        const SegInfo info = analyse_segment(s, i);
        uint32_t error = info.error;
        if (!error) {
            const bool neighbour = i + 1 < s.n && integral_same_group(groups, i, i + 1);
            transit_segment(s, i, info, q, b_first, count, (uint64_t)group * q.buckets.n_buckets, lane, cells, neighbour,
                            heads, &error);
        }
        errors |= error;
    }
    lane.flush();
    if (errors) atomicOr(error_word, errors);
}

namespace {

// One pass: the linked pairs of the device batch `in` (groups: a device array or nullptr) inside the request's
// buckets, counted into zeroed scratch counters and then ADDED to dev_counts (a device array) or host_counts (the
// caller's, after one download) - only once the pass is known to be free of errors.
int transit_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_transit_request *request,
                const std::vector<int32_t> &edge_keys, uint64_t n_rows, unsigned long long *dev_counts,
                uint64_t *host_counts) {
    const uint64_t n = in->n;
    if (n == 0 || n_rows == 0) return 0;
    const mdb_bucket_request &b = request->buckets;
    // (the span, the heads and the rows are the time-weighted operator's: its request with a method nobody reads)
    const IntegralRequest q = {{b.origin, b.width, b.n_buckets, b.t_lo, b.t_hi, b.n_groups, b.which_mask},
                               request->max_gap, 0u};
    const uint64_t n_cells = edge_keys.size() + 1;
    const uint64_t total = n_rows * n_cells * n_cells;
    if (hist_buckets_fits(total * 8, "n_groups * n_buckets * n_cells * n_cells counters")) return 1;
    const DevSegments s = to_dev(in);
    void *p = nullptr;
    const uint64_t cells_bytes = align_up(total * 8, 256), keys_bytes = align_up(edge_keys.size() * 4, 256);
    if (scratch_reserve(ctx, SCRATCH_HIST_CELLS, cells_bytes + keys_bytes + 256, &p)) return 1;
    Carver scratch(p);
    unsigned long long *cells = scratch.take<unsigned long long>(total);
    int32_t *keys = scratch.take<int32_t>(edge_keys.size());
    unsigned int *words = scratch.take<unsigned int>(2);
    if (scratch_reserve(ctx, SCRATCH_INTEGRAL_HEADS, n * sizeof(IntegralHead), &p)) return 1;
    IntegralHead *heads = static_cast<IntegralHead *>(p);
    MDB_HIP_CHECK(hipMemsetAsync(cells, 0, total * 8, ctx->stream));
    MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
    MDB_HIP_CHECK(mail_write(ctx, keys, edge_keys.data(), edge_keys.size() * 4));
    if (groups) hist_groups_launch(ctx, groups, n, q.buckets.n_groups, words);
    {
        LaunchTimer timer(ctx, "k_transit_heads");
        hipLaunchKernelGGL(k_transit_heads, dim3((uint32_t)((n + HIST_THREADS - 1) / HIST_THREADS)), dim3(HIST_THREADS), 0,
                           ctx->stream, s, groups, q, heads, words);
    }
    {
        LaunchTimer timer(ctx, "k_transit_buckets");
        hipLaunchKernelGGL(k_transit_buckets, dim3(hist_blocks(n)), dim3(HIST_THREADS), 0, ctx->stream, s, groups, q, keys,
                           (uint32_t)edge_keys.size(), heads, cells, words);
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
        transit_merge(host_counts, added.data(), total);
        return 0;
    }
    hist_fold_launch(ctx, cells, total, dev_counts);
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    return 0;
}

} // namespace

int transit_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                     uint32_t n_inputs, const mdb_transit_request *request, const std::vector<int32_t> &edge_keys,
                     uint64_t n_rows, uint64_t *counts) {
    // (into the context's upload scratch, as mdb_dwell_buckets_list: the host and device forms run the same kernels)
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, true)) return 1;
    return transit_run(ctx, list.segments(), list.groups(), request, edge_keys, n_rows, nullptr, counts);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_transit_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                                       const mdb_transit_request *request, const float *edges, uint32_t n_edges,
                                       uint64_t *counts) {
    if (!ctx || !in || !request || !edges || !counts) return fail("ctx, in, request, edges and counts must not be NULL.");
    std::vector<int32_t> edge_keys;
    uint64_t n_rows = 0;
    if (hist_edge_keys(edges, n_edges, &edge_keys)) return 1;
    if (transit_request_check(request, n_edges, &n_rows)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return transit_run(ctx, in, group_of_segment, request, edge_keys, n_rows, reinterpret_cast<unsigned long long *>(counts),
                       nullptr);
}
