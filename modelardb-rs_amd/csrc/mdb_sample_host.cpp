// mdb_sample_host.cpp - the entry points of the sampling operator that take host batches, up to the point where the
// device is needed (sample_list_run, mdb_sample.hip), and the host arithmetic on cells: mdb_sample_merge_n and
// mdb_sample_values. Plain C++, no HIP type: the check program tests/sample_host builds this file with g++ under the
// CPU sanitizers against a stand-in for sample_list_run.
#include "mdb_sample.hpp"

#include <limits>

using namespace mdb;

extern "C" {

int mdb_sample_at_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                       uint32_t n_inputs, const mdb_sample_request *request, mdb_sample_cell *inout) {
    if (!ctx || !inputs || !request || !inout) return fail("ctx, inputs, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (sample_request_check(request, &n_cells)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || request->instants.n_buckets == 0) return 0;
    return sample_list_run(ctx, inputs, group_of_segment, n_inputs, request, n_cells, inout);
}

int mdb_sample_at(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                  const mdb_sample_request *request, mdb_sample_cell *inout) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_sample_at_list(ctx, &in, groups, 1, request, inout);
}

int mdb_sample_merge_n(mdb_sample_cell *into, const mdb_sample_cell *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    for (uint64_t j = 0; j < n; j++) sample_cell_add(into[j], from[j]);
    return 0;
}

int mdb_sample_values(const mdb_sample_cell *cells, uint64_t n, double *out) {
    if (n > 0 && (!cells || !out)) return fail("cells and out must not be NULL.");
    for (uint64_t j = 0; j < n; j++)
        out[j] = cells[j].count == 0 ? std::numeric_limits<double>::quiet_NaN() : cells[j].sum / (double)cells[j].count;
    return 0;
}

} // extern "C"
