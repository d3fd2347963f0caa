// mdb_derived_host.cpp - the entry points of the derived-field operator that take host batches, up to the point where
// the device is needed (derived_list_run, derived_values_host_run: mdb_derived.hip), and the host arithmetic:
// mdb_derived_apply, mdb_derived_merge_n and mdb_derived_stats. Plain C++, no HIP type: the check program
// tests/derived_host builds this file with g++ under the CPU sanitizers against stand-ins for the two device steps.
#include "mdb_derived.hpp"

using namespace mdb;

extern "C" {

int mdb_derived_buckets_list(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                             uint32_t n_y, const uint32_t *const *group_of_segment_x,
                             const mdb_bucket_request *request, const mdb_derived_expr *expr, mdb_derived_cell *inout) {
    if (!ctx || !xs || !ys || !request || !expr || !inout)
        return fail("ctx, xs, ys, request, expr and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (derived_request_check(request, &n_cells) || derived_expr_check(expr)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_x; k++) {
        if (!xs[k]) return fail("A batch of the list xs is NULL.");
        n += xs[k]->n;
    }
    for (uint32_t k = 0; k < n_y; k++)
        if (!ys[k]) return fail("A batch of the list ys is NULL.");
    if (n == 0 || request->n_buckets == 0) return 0;
    return derived_list_run(ctx, xs, n_x, ys, n_y, group_of_segment_x, request, expr, n_cells, inout);
}

int mdb_derived_buckets(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const uint32_t *group_of_segment_x,
                        const mdb_bucket_request *request, const mdb_derived_expr *expr, mdb_derived_cell *inout) {
    if (!x || !y) return fail("x and y must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment_x};
    return mdb_derived_buckets_list(ctx, &x, 1, &y, 1, groups, request, expr, inout);
}

int mdb_derived_values(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const mdb_derived_expr *expr,
                       int64_t t_lo, int64_t t_hi, int64_t *timestamps, float *values, uint64_t capacity,
                       uint64_t *rows_out) {
    if (!ctx || !x || !y || !expr || !rows_out) return fail("ctx, x, y, expr and rows_out must not be NULL.");
    if (derived_expr_check(expr)) return 1;
    if (x->n == 0 || t_lo > t_hi) {
        *rows_out = 0;
        return 0;
    }
    return derived_values_host_run(ctx, x, y, expr, t_lo, t_hi, timestamps, values, capacity, rows_out);
}

int mdb_derived_apply(const mdb_derived_expr *expr, const float *x, const float *y, uint64_t n, float *z) {
    if (!expr) return fail("expr must not be NULL.");
    if (derived_expr_check(expr)) return 1;
    if (n > 0 && (!x || !y || !z)) return fail("x, y and z must not be NULL.");
    const mdb_derived_expr e = *expr;
    for (uint64_t j = 0; j < n; j++) z[j] = derived_eval(e, x[j], y[j]);
    return 0;
}

int mdb_derived_merge_n(mdb_derived_cell *into, const mdb_derived_cell *from, uint64_t n) {
    if (n > 0 && (!into || !from)) return fail("into and from must not be NULL.");
    for (uint64_t j = 0; j < n; j++) derived_merge(into[j], from[j]);
    return 0;
}

int mdb_derived_stats(const mdb_derived_cell *cells, uint64_t n, mdb_moments_cell *out) {
    if (n > 0 && (!cells || !out)) return fail("cells and out must not be NULL.");
    for (uint64_t j = 0; j < n; j++) {
        const mdb_derived_cell &cell = cells[j];
        if (cell.count == 0) out[j] = mdb_moments_cell{0, 0.0, 0.0}; // (an empty cell: no other member is read)
        else out[j] = mdb_moments_cell{cell.count, cell.mean, cell.m2};
    }
    return 0;
}

} // extern "C"
