// mdb_comoments_host.cpp - the entry points of the covariance operator that take host batches, up to the point where
// the device is needed (comoments_list_run, mdb_comoments.hip), and the host arithmetic on cells:
// mdb_comoments_merge_n, mdb_comoments_moments and mdb_comoments_finish. Plain C++, no HIP type: the check program
// tests/comoments_host builds this file with g++ under the CPU sanitizers against a stand-in for comoments_list_run.
#include "mdb_comoments.hpp"

using namespace mdb;

extern "C" {

int mdb_comoments_buckets_list(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                               uint32_t n_y, const uint32_t *const *group_of_segment_x,
                               const mdb_bucket_request *request, mdb_comoments_cell *inout) {
    if (!ctx || !xs || !ys || !request || !inout) return fail("ctx, xs, ys, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (comoments_request_check(request, &n_cells)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_x; k++) {
        if (!xs[k]) return fail("A batch of the list xs is NULL.");
        n += xs[k]->n;
    }
    for (uint32_t k = 0; k < n_y; k++)
        if (!ys[k]) return fail("A batch of the list ys is NULL.");
    if (n == 0 || request->n_buckets == 0) return 0;
    return comoments_list_run(ctx, xs, n_x, ys, n_y, group_of_segment_x, request, n_cells, inout);
}

int mdb_comoments_buckets(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const uint32_t *group_of_segment_x,
                          const mdb_bucket_request *request, mdb_comoments_cell *inout) {
    if (!x || !y) return fail("x and y must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment_x};
    return mdb_comoments_buckets_list(ctx, &x, 1, &y, 1, groups, request, inout);
}

int mdb_comoments_merge_n(mdb_comoments_cell *into, const mdb_comoments_cell *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    for (uint64_t j = 0; j < n; j++) comoments_merge(into[j], from[j]);
    return 0;
}

int mdb_comoments_moments(const mdb_comoments_cell *cells, uint64_t n, uint32_t which, mdb_moments_cell *out) {
    if (which > 1) return fail("which must be 0 (the x field) or 1 (the y field).");
    if (n > 0 && (!cells || !out)) return fail("cells and out must not be NULL.");
    for (uint64_t j = 0; j < n; j++) {
        const mdb_comoments_cell &cell = cells[j];
        if (cell.count == 0) out[j] = mdb_moments_cell{0, 0.0, 0.0}; // (an empty cell: no other member is read)
        else out[j] = mdb_moments_cell{cell.count, which == 0 ? cell.mean_x : cell.mean_y, which == 0 ? cell.m2_x : cell.m2_y};
    }
    return 0;
}

int mdb_comoments_finish(const mdb_comoments_cell *cells, uint64_t n, uint32_t kind, double *out) {
    if (kind > MDB_COMOMENTS_REGR_R2) return fail("Unknown kind " + std::to_string(kind) + " (MDB_COMOMENTS_*).");
    if (n > 0 && (!cells || !out)) return fail("cells and out must not be NULL.");
    for (uint64_t j = 0; j < n; j++) out[j] = comoments_statistic(cells[j], kind);
    return 0;
}

} // extern "C"
