// mdb_dwell.hip - the time spent per value cell, per date_bin bucket and group, computed on segments
// (mdb_dwell_buckets*): dwell[group][bucket][cell] in microseconds, in one pass over the batch.
//
// What the reference can only answer with GridExec -> WindowAggExec(lag) -> AggregateExec GROUP BY date_bin,
// width_bucket over every rebuilt point. Here a (segment, bucket) pair is one add for PMC-Mean and the binary searches
// of k_hist_buckets for Swing on regular timestamps. k_hist_buckets' shape with the time-weighted operator's extent:
//
//   k_hist_groups    (mdb_hist.hip) every row's group id checked, also the rows the request leaves out.
//   k_dwell_buckets  1 lane / segment, grid-strided and launched like k_hist_buckets, the edges' keys in LDS. The
//                    lane's buckets are those its extent [start_time, linked ? start_time of the next : end_time]
//                    overlaps (integral_span): the link to the right neighbour belongs to the left segment, and only
//                    the neighbour's start_time and group are read for it. What a lane makes of its segment is
//                    mdb_dwell.hpp's dwell_segment; its run is flushed wherever the (group, bucket) row, the cell or
//                    the unit changes.
//   k_hist_fold      (mdb_hist.hip) the scratch counters added into the caller's (the _dev form).
// Integers only, integer atomics on zeroed scratch counters, which are added to the caller's array only once the
// error word has been read back clean: the forms and any two runs agree bit for bit. Every stream is one lane's: the
// batch's cursor index is not used (as k_hist_buckets).
//
// Scratch: 8 B per counter, the edges' keys and the error word (SCRATCH_HIST_CELLS, as mdb_hist_buckets).
#include "mdb_dwell.hpp"

#include <vector>

namespace mdb {

// cells: n_groups * n_buckets rows of n_edges + 1 zeroed counters. (A row with a bad group id is skipped here as well:
// nothing is ever added outside the cells, whatever k_hist_groups has found.)
__global__ __launch_bounds__(HIST_THREADS) void k_dwell_buckets(DevSegments s, const uint32_t *__restrict__ groups,
                                                                IntegralRequest q, const int32_t *__restrict__ edge_keys,
                                                                uint32_t n_edges, unsigned long long *__restrict__ cells,
                                                                unsigned int *__restrict__ error_word) {
    __shared__ int32_t lds_keys[MDB_HIST_MAX_EDGES + 1];
    for (uint32_t j = threadIdx.x; j < n_edges; j += HIST_THREADS) lds_keys[j] = edge_keys[j];
    __syncthreads();
    DwellLane lane = {lds_keys, n_edges, cells, 1, 0, 0, 0, 1};
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
        if (!error) dwell_segment(s, groups, i, info, q, b_first, count, (uint64_t)group * q.buckets.n_buckets, lane, cells, &error);
        errors |= error;
    }
    lane.flush();
    if (errors) atomicOr(error_word, errors);
}

namespace {

// One pass: the linked time of the device batch `in` (groups: a device array or nullptr) inside the request's buckets,
// counted into zeroed scratch counters and then ADDED to dev_dwell (a device array) or host_dwell (the caller's, after
// one download) - only once the pass is known to be free of errors.
int dwell_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_dwell_request *request,
              const std::vector<int32_t> &edge_keys, uint64_t n_rows, unsigned long long *dev_dwell, uint64_t *host_dwell) {
    const uint64_t n = in->n;
    if (n == 0 || n_rows == 0) return 0;
    const mdb_bucket_request &b = request->buckets;
    const IntegralRequest q = {{b.origin, b.width, b.n_buckets, b.t_lo, b.t_hi, b.n_groups, b.which_mask},
                               request->max_gap, MDB_INTEGRAL_STEP};
    const uint64_t total = n_rows * (edge_keys.size() + 1);
    if (hist_buckets_fits(total * 8, "n_groups * n_buckets * n_cells counters")) return 1;
    const DevSegments s = to_dev(in);
    void *p = nullptr;
    const uint64_t cells_bytes = align_up(total * 8, 256), keys_bytes = align_up(edge_keys.size() * 4, 256);
    if (scratch_reserve(ctx, SCRATCH_HIST_CELLS, cells_bytes + keys_bytes + 256, &p)) return 1;
    Carver scratch(p);
    unsigned long long *cells = scratch.take<unsigned long long>(total);
    int32_t *keys = scratch.take<int32_t>(edge_keys.size());
    unsigned int *words = scratch.take<unsigned int>(2);
    MDB_HIP_CHECK(hipMemsetAsync(cells, 0, total * 8, ctx->stream));
    MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
    MDB_HIP_CHECK(mail_write(ctx, keys, edge_keys.data(), edge_keys.size() * 4));
    if (groups) hist_groups_launch(ctx, groups, n, q.buckets.n_groups, words);
    {
        LaunchTimer timer(ctx, "k_dwell_buckets");
        hipLaunchKernelGGL(k_dwell_buckets, dim3(hist_blocks(n)), dim3(HIST_THREADS), 0, ctx->stream, s, groups, q, keys,
                           (uint32_t)edge_keys.size(), cells, words);
    }
    unsigned int error = 0;
    MDB_HIP_CHECK(hipMemcpyAsync(&error, words, 4, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (error & ERR_HIST_GROUP) return fail("A group id is not below n_groups.");
    if (error) return fail(describe_error(error));
    if (host_dwell) {
        std::vector<uint64_t> added(total);
        MDB_HIP_CHECK(hipMemcpyAsync(added.data(), cells, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (uint64_t j = 0; j < total; j++) host_dwell[j] += added[j];
        return 0;
    }
    hist_fold_launch(ctx, cells, total, dev_dwell);
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    return 0;
}

} // namespace

int dwell_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                   uint32_t n_inputs, const mdb_dwell_request *request, const std::vector<int32_t> &edge_keys,
                   uint64_t n_rows, uint64_t *dwell) {
    // (into the context's upload scratch, as mdb_hist_buckets_list: the host and device forms run the same kernel)
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, true)) return 1;
    return dwell_run(ctx, list.segments(), list.groups(), request, edge_keys, n_rows, nullptr, dwell);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_dwell_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                                     const mdb_dwell_request *request, const float *edges, uint32_t n_edges, uint64_t *dwell) {
    if (!ctx || !in || !request || !edges || !dwell) return fail("ctx, in, request, edges and dwell must not be NULL.");
    std::vector<int32_t> edge_keys;
    uint64_t n_rows = 0;
    if (hist_edge_keys(edges, n_edges, &edge_keys)) return 1;
    if (dwell_request_check(request, n_edges, &n_rows)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return dwell_run(ctx, in, group_of_segment, request, edge_keys, n_rows, reinterpret_cast<unsigned long long *>(dwell),
                     nullptr);
}
