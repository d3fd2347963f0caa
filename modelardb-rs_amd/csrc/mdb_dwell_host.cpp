// mdb_dwell_host.cpp - the entry points of the dwell operator that take host batches, up to the point where the device
// is needed (dwell_list_run, mdb_dwell.hip), and the host arithmetic on its counters: mdb_dwell_merge_n and
// mdb_dwell_share. Plain C++, no HIP type: the check program tests/dwell_host builds this file with g++ under the CPU
// sanitizers against a stand-in for dwell_list_run.
#include "mdb_dwell.hpp"

#include <limits>

using namespace mdb;

extern "C" {

int mdb_dwell_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                           uint32_t n_inputs, const mdb_dwell_request *request, const float *edges, uint32_t n_edges,
                           uint64_t *dwell) {
    if (!ctx || !inputs || !request || !edges || !dwell)
        return fail("ctx, inputs, request, edges and dwell must not be NULL.");
    std::vector<int32_t> edge_keys;
    uint64_t n_rows = 0;
    if (hist_edge_keys(edges, n_edges, &edge_keys)) return 1;
    if (dwell_request_check(request, n_edges, &n_rows)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || n_rows == 0) return 0;
    return dwell_list_run(ctx, inputs, group_of_segment, n_inputs, request, edge_keys, n_rows, dwell);
}

int mdb_dwell_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                      const mdb_dwell_request *request, const float *edges, uint32_t n_edges, uint64_t *dwell) {
    if (!in) return fail("ctx, in, request, edges and dwell must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_dwell_buckets_list(ctx, &in, groups, 1, request, edges, n_edges, dwell);
}

int mdb_dwell_merge_n(uint64_t *into, const uint64_t *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    for (uint64_t j = 0; j < n; j++) into[j] += from[j];
    return 0;
}

int mdb_dwell_share(const uint64_t *dwell, uint64_t n_rows, uint32_t n_cells, double *out) {
    if (n_rows > 0 && n_cells > 0 && (!dwell || !out)) return fail("dwell and out must not be NULL.");
    for (uint64_t row = 0; row < n_rows; row++) {
        const uint64_t *cells = dwell + row * n_cells;
        // (a row's total is at most the bucket's width times the rows of the group that overlap it: the sum is formed
        // in 128 bits so that merged arrays cannot wrap it either)
        unsigned __int128 total = 0;
        for (uint32_t c = 0; c < n_cells; c++) total += cells[c];
        for (uint32_t c = 0; c < n_cells; c++)
            out[row * n_cells + c] = total == 0 ? std::numeric_limits<double>::quiet_NaN() : (double)cells[c] / (double)total;
    }
    return 0;
}

} // extern "C"
