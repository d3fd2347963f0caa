// mdb_transit_host.cpp - the entry points of the transitions operator that take host batches, up to the point where the
// device is needed (transit_list_run, mdb_transit.hip), and the host arithmetic on its counters: mdb_transit_merge_n
// and mdb_transit_crossings. Plain C++, no HIP type: the check program tests/transit_host builds this file with g++
// under the CPU sanitizers against a stand-in for transit_list_run.
#include "mdb_transit.hpp"

using namespace mdb;

extern "C" {

int mdb_transit_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                             uint32_t n_inputs, const mdb_transit_request *request, const float *edges, uint32_t n_edges,
                             uint64_t *counts) {
    if (!ctx || !inputs || !request || !edges || !counts)
        return fail("ctx, inputs, request, edges and counts must not be NULL.");
    std::vector<int32_t> edge_keys;
    uint64_t n_rows = 0;
    if (hist_edge_keys(edges, n_edges, &edge_keys)) return 1;
    if (transit_request_check(request, n_edges, &n_rows)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || n_rows == 0) return 0;
    return transit_list_run(ctx, inputs, group_of_segment, n_inputs, request, edge_keys, n_rows, counts);
}

int mdb_transit_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                        const mdb_transit_request *request, const float *edges, uint32_t n_edges, uint64_t *counts) {
    if (!in) return fail("ctx, in, request, edges and counts must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_transit_buckets_list(ctx, &in, groups, 1, request, edges, n_edges, counts);
}

int mdb_transit_merge_n(uint64_t *into, const uint64_t *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    transit_merge(into, from, n);
    return 0;
}

int mdb_transit_crossings(const uint64_t *counts, uint64_t n_rows, uint32_t n_cells, uint64_t *up, uint64_t *down) {
    if (n_cells < 1) return fail("n_cells must be at least 1.");
    if (n_rows > 0 && (!counts || (n_cells > 1 && (!up || !down)))) return fail("counts, up and down must not be NULL.");
    transit_crossings(counts, n_rows, n_cells, up, down);
    return 0;
}

} // extern "C"
