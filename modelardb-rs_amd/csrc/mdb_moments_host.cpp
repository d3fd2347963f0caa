// mdb_moments_host.cpp - the entry points of the variance operator that take host batches, up to the point where the
// device is needed (moments_list_run, mdb_moments.hip), and the host arithmetic on cells: mdb_moments_merge_n and
// mdb_moments_variance. Plain C++, no HIP type: the check program tests/moments_host builds this file with g++ under
// the CPU sanitizers against a stand-in for moments_list_run.
#include "mdb_moments.hpp"

#include <limits>

using namespace mdb;

extern "C" {

int mdb_moments_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                             uint32_t n_inputs, const mdb_bucket_request *request, mdb_moments_cell *inout) {
    if (!ctx || !inputs || !request || !inout) return fail("ctx, inputs, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (moments_request_check(request, &n_cells)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || request->n_buckets == 0) return 0;
    return moments_list_run(ctx, inputs, group_of_segment, n_inputs, request, n_cells, inout);
}

int mdb_moments_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                        const mdb_bucket_request *request, mdb_moments_cell *inout) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_moments_buckets_list(ctx, &in, groups, 1, request, inout);
}

int mdb_moments_merge_n(mdb_moments_cell *into, const mdb_moments_cell *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    for (uint64_t j = 0; j < n; j++) moments_merge(into[j], from[j]);
    return 0;
}

int mdb_moments_variance(const mdb_moments_cell *cells, uint64_t n, uint32_t ddof, double *variance_out) {
    if (ddof > 1) return fail("ddof must be 0 (population) or 1 (sample).");
    if (n > 0 && (!cells || !variance_out)) return fail("cells and variance_out must not be NULL.");
    for (uint64_t j = 0; j < n; j++) {
        const int64_t count = cells[j].count;
        variance_out[j] = count <= (int64_t)ddof ? std::numeric_limits<double>::quiet_NaN()
                                                 : cells[j].m2 / (double)(count - (int64_t)ddof);
    }
    return 0;
}

} // extern "C"
