// mdb_change_host.cpp - the entry points of the change operator that take host batches, up to the point where the
// device is needed (change_list_run, mdb_change.hip), and the host arithmetic on cells: mdb_change_merge_n and
// mdb_change_finish. Plain C++, no HIP type: the check program tests/change_host builds this file with g++ under the
// CPU sanitizers against a stand-in for change_list_run.
#include "mdb_change.hpp"

#include <limits>

using namespace mdb;

extern "C" {

int mdb_change_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                            uint32_t n_inputs, const mdb_change_request *request, mdb_change_cell *inout) {
    if (!ctx || !inputs || !request || !inout) return fail("ctx, inputs, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (change_request_check(request, &n_cells)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || request->buckets.n_buckets == 0) return 0;
    return change_list_run(ctx, inputs, group_of_segment, n_inputs, request, n_cells, inout);
}

int mdb_change_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                       const mdb_change_request *request, mdb_change_cell *inout) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_change_buckets_list(ctx, &in, groups, 1, request, inout);
}

int mdb_change_merge_n(mdb_change_cell *into, const mdb_change_cell *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    for (uint64_t j = 0; j < n; j++) change_cell_merge(into[j], from[j]);
    return 0;
}

int mdb_change_finish(const mdb_change_cell *cells, uint64_t n, uint32_t kind, double *out) {
    if (kind != MDB_CHANGE_NET && kind != MDB_CHANGE_VARIATION && kind != MDB_CHANGE_INCREASE && kind != MDB_CHANGE_RATE)
        return fail("Unknown kind: MDB_CHANGE_NET, _VARIATION, _INCREASE or _RATE.");
    if (n > 0 && (!cells || !out)) return fail("cells and out must not be NULL.");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint64_t j = 0; j < n; j++) {
        const mdb_change_cell &c = cells[j];
        if (c.count == 0) out[j] = nan;
        else if (kind == MDB_CHANGE_NET) out[j] = c.rise - c.fall;
        else if (kind == MDB_CHANGE_VARIATION) out[j] = c.rise + c.fall;
        else if (kind == MDB_CHANGE_INCREASE) out[j] = c.rise + c.reset_sum;
        else out[j] = c.duration == 0 ? nan : (c.rise + c.reset_sum) * 1e6 / (double)c.duration;
    }
    return 0;
}

} // extern "C"
