// mdb_m4_host.cpp - the entry points of M4 downsampling that take host batches, up to the point where the device is
// needed (m4_list_run, mdb_m4.hip), and mdb_m4_merge_n. Plain C++, no HIP type: the check program tests/m4_host builds
// this file with g++ under the CPU sanitizers against a stand-in for m4_list_run.
#include "mdb_m4.hpp"

using namespace mdb;

extern "C" {

int mdb_m4_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                        uint32_t n_inputs, const mdb_bucket_request *request, mdb_m4_cell *inout) {
    if (!ctx || !inputs || !request || !inout) return fail("ctx, inputs, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (m4_request_check(request, &n_cells)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || request->n_buckets == 0) return 0;
    return m4_list_run(ctx, inputs, group_of_segment, n_inputs, request, n_cells, inout);
}

int mdb_m4_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                   const mdb_bucket_request *request, mdb_m4_cell *inout) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_m4_buckets_list(ctx, &in, groups, 1, request, inout);
}

int mdb_m4_merge_n(mdb_m4_cell *into, const mdb_m4_cell *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    for (uint64_t j = 0; j < n; j++) m4_merge(into[j], from[j]);
    return 0;
}

} // extern "C"
