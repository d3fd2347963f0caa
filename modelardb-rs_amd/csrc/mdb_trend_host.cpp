// mdb_trend_host.cpp - the entry points of the trend operator that take host batches, up to the point where the device
// is needed (trend_list_run, mdb_trend.hip). The cells are mdb_comoments_cell: mdb_comoments_merge_n, _moments and
// _finish (mdb_comoments_host.cpp) are the host arithmetic, there is none of its own here. Plain C++, no HIP type: the
// check program tests/trend_host builds this file with g++ under the CPU sanitizers against a stand-in for
// trend_list_run.
#include "mdb_trend.hpp"

using namespace mdb;

extern "C" {

int mdb_trend_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                           uint32_t n_inputs, const mdb_bucket_request *request, mdb_comoments_cell *inout) {
    if (!ctx || !inputs || !request || !inout) return fail("ctx, inputs, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (trend_request_check(request, &n_cells)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || request->n_buckets == 0) return 0;
    return trend_list_run(ctx, inputs, group_of_segment, n_inputs, request, n_cells, inout);
}

int mdb_trend_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                      const mdb_bucket_request *request, mdb_comoments_cell *inout) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_trend_buckets_list(ctx, &in, groups, 1, request, inout);
}

} // extern "C"
