// mdb_integral_host.cpp - the entry points of the time-weighted operator that take host batches, up to the point where
// the device is needed (integral_list_run, mdb_integral.hip), and the host arithmetic on cells: mdb_integral_merge_n
// and mdb_integral_average. Plain C++, no HIP type: the check program tests/integral_host builds this file with g++
// under the CPU sanitizers against a stand-in for integral_list_run.
#include "mdb_integral.hpp"

#include <limits>

using namespace mdb;

extern "C" {

int mdb_integral_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                              uint32_t n_inputs, const mdb_integral_request *request, mdb_integral_cell *inout) {
    if (!ctx || !inputs || !request || !inout) return fail("ctx, inputs, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (integral_request_check(request, &n_cells)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || request->buckets.n_buckets == 0) return 0;
    return integral_list_run(ctx, inputs, group_of_segment, n_inputs, request, n_cells, inout);
}

int mdb_integral_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                         const mdb_integral_request *request, mdb_integral_cell *inout) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_integral_buckets_list(ctx, &in, groups, 1, request, inout);
}

int mdb_integral_merge_n(mdb_integral_cell *into, const mdb_integral_cell *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    for (uint64_t j = 0; j < n; j++) integral_cell_add(into[j], from[j]);
    return 0;
}

int mdb_integral_average(const mdb_integral_cell *cells, uint64_t n, double *out) {
    if (n > 0 && (!cells || !out)) return fail("cells and out must not be NULL.");
    for (uint64_t j = 0; j < n; j++)
        out[j] = cells[j].duration == 0 ? std::numeric_limits<double>::quiet_NaN()
                                        : cells[j].integral / (double)cells[j].duration;
    return 0;
}

} // extern "C"
