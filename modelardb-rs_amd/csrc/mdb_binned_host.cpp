// mdb_binned_host.cpp - the entry points of mdb_binned_buckets* that take host batches, up to the point where the
// device is needed (binned_list_run, mdb_binned.hip). Plain C++, no HIP type: the check program tests/binned_host
// builds this file with g++ under the CPU sanitizers against a stand-in for binned_list_run.
#include "mdb_binned.hpp"

using namespace mdb;

extern "C" {

int mdb_binned_buckets_list(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                            uint32_t n_y, const uint32_t *const *group_of_segment_x, const mdb_bucket_request *request,
                            const float *edges, uint32_t n_edges, mdb_moments_cell *inout) {
    if (!ctx || !xs || !ys || !request || !edges || !inout)
        return fail("ctx, xs, ys, request, edges and inout must not be NULL.");
    std::vector<int32_t> edge_keys;
    uint64_t n_cells = 0;
    if (binned_arguments_check(request, edges, n_edges, &edge_keys, &n_cells)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_x; k++) {
        if (!xs[k]) return fail("A batch of the list xs is NULL.");
        n += xs[k]->n;
    }
    for (uint32_t k = 0; k < n_y; k++)
        if (!ys[k]) return fail("A batch of the list ys is NULL.");
    if (n == 0 || request->n_buckets == 0) return 0;
    return binned_list_run(ctx, xs, n_x, ys, n_y, group_of_segment_x, request, edge_keys, n_cells, inout);
}

int mdb_binned_buckets(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const uint32_t *group_of_segment_x,
                       const mdb_bucket_request *request, const float *edges, uint32_t n_edges, mdb_moments_cell *inout) {
    if (!x || !y) return fail("x and y must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment_x};
    return mdb_binned_buckets_list(ctx, &x, 1, &y, 1, groups, request, edges, n_edges, inout);
}

} // extern "C"
