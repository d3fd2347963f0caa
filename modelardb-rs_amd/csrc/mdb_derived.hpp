// mdb_derived.hpp - derived fields of two fields (mdb_derived_*): z = f(x, y) as a column and, per date_bin bucket and
// group, the count, mean, m2, min and max of z.
//
// Plain C++ (no HIP type): the evaluator of an mdb_derived_expr, a run of z values accumulated with shifted sums and
// running extremes, the merge rule on cells and the checks of an expression and a request. ONE evaluator
// (derived_eval) is shared by the kernels (mdb_derived.hip), by the host entry points (mdb_derived_host.cpp) and by
// the check program tests/derived_host, which runs all of this under the CPU sanitizers.
//
// The arithmetic of z: every operation is one binary32 operation in the written order. The translation units that
// include this header are built with -ffp-contract=off (and, on the device, without flushing denormals), so nothing is
// fused and the division is the correctly rounded one. Zeros follow from the formula as written: c = +0 turns a -0 sum
// into +0; nothing is special-cased.
//
// A run is summed around its first z exactly as mdb_moments.hpp sums a run around its first value; min and max take a
// value by the rule of mdb_agg_buckets' MIN and MAX (RangeAcc::point, min_num / max_num of mdb_common.hpp): they start
// at FLT_MAX / -FLT_MAX, a NaN is skipped, and of -0.0 and +0.0 the one met first stays.
#pragma once

#include "mdb_moments.hpp"

#include <cfloat>
#include <cmath>
#include <string>

namespace mdb {

// z = f(x, y). The expression has been checked (derived_expr_check): op is one of the three.
MDB_MOMENTS_FN float derived_eval(const mdb_derived_expr &e, float x, float y) {
    float z;
    if (e.op == MDB_DERIVED_LINEAR) {
        const float ax = e.a * x;
        const float by = e.b * y;
        const float sum = ax + by;
        z = sum + e.c;
    } else {
        const float inner = e.op == MDB_DERIVED_PRODUCT ? x * y : x / y;
        const float scaled = e.a * inner;
        z = scaled + e.c;
    }
    if (e.flags & MDB_DERIVED_ABS) {
        uint32_t bits;
        __builtin_memcpy(&bits, &z, 4);
        bits &= 0x7fffffffu;
        __builtin_memcpy(&z, &bits, 4);
    }
    return z;
}

// min_num / max_num of mdb_common.hpp (device only there), for host and device: `a` is the extreme so far.
MDB_MOMENTS_FN float derived_min(float a, float b) {
    if (a != a) return b;
    return (b < a) ? b : a;
}
MDB_MOMENTS_FN float derived_max(float a, float b) {
    if (a != a) return b;
    return (b > a) ? b : a;
}

struct DerivedRun {
    MomentsRun moments;
    float min, max;
};

MDB_MOMENTS_FN DerivedRun derived_run_empty() { return DerivedRun{moments_run_empty(), FLT_MAX, -FLT_MAX}; }

MDB_MOMENTS_FN void derived_point(DerivedRun &run, float z) {
    moments_point(run.moments, z);
    run.min = derived_min(run.min, z);
    run.max = derived_max(run.max, z);
}

// The cell of a run; an empty run gives a fresh cell (all-zero bytes).
MDB_MOMENTS_FN mdb_derived_cell derived_finish(const DerivedRun &run) {
    mdb_derived_cell cell = {0, 0.0, 0.0, 0.0f, 0.0f};
    if (run.moments.n == 0) return cell;
    const mdb_moments_cell m = moments_finish(run.moments);
    cell.count = m.count;
    cell.mean = m.mean;
    cell.m2 = m.m2;
    cell.min = run.min;
    cell.max = run.max;
    return cell;
}

// The values of `from` added to those of `into`. An empty `from` changes nothing; an empty `into` (count 0: no other
// member is read) takes every member of `from`. count, mean and m2: moments_merge. min, max: `into` holds the extreme
// so far.
MDB_MOMENTS_FN void derived_merge(mdb_derived_cell &into, const mdb_derived_cell &from) {
    if (from.count == 0) return;
    if (into.count == 0) {
        into = from;
        return;
    }
    mdb_moments_cell a = {into.count, into.mean, into.m2};
    moments_merge(a, mdb_moments_cell{from.count, from.mean, from.m2});
    into.count = a.count;
    into.mean = a.mean;
    into.m2 = a.m2;
    into.min = derived_min(into.min, from.min);
    into.max = derived_max(into.max, from.max);
}

inline int derived_expr_check(const mdb_derived_expr *expr) {
    if (expr->op > MDB_DERIVED_RATIO) return fail("Unknown op " + std::to_string(expr->op) + " (MDB_DERIVED_LINEAR, _PRODUCT or _RATIO).");
    if (expr->flags & ~MDB_DERIVED_ABS) return fail("Unknown flag bits " + std::to_string(expr->flags) + " in mdb_derived_expr (MDB_DERIVED_ABS).");
    if (!std::isfinite(expr->a) || !std::isfinite(expr->b) || !std::isfinite(expr->c))
        return fail("The coefficients a, b and c of mdb_derived_expr must be finite.");
    return 0;
}

// The host-side checks every form makes before it touches the device: those of mdb_moments_buckets*.
inline int derived_request_check(const mdb_bucket_request *request, uint64_t *n_cells) {
    if (request->which_mask != 0) return fail("which_mask must be 0 for mdb_derived_buckets*.");
    if (request->width <= 0) return fail("The bucket width must be positive.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    const unsigned __int128 cells = (unsigned __int128)request->n_groups * request->n_buckets;
    if (cells * sizeof(mdb_derived_cell) > (unsigned __int128)UINT64_MAX) return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// mdb_derived.hip: the host batches of the two lists uploaded (a batch that is in both lists once) and folded into the
// caller's cells / rebuilt into the caller's host arrays (expression and request checked, xs not empty). The only
// steps of the host forms that need the device.
int derived_list_run(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                     uint32_t n_y, const uint32_t *const *group_of_segment_x, const mdb_bucket_request *request,
                     const mdb_derived_expr *expr, uint64_t n_cells, mdb_derived_cell *inout);
int derived_values_host_run(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const mdb_derived_expr *expr,
                            int64_t t_lo, int64_t t_hi, int64_t *timestamps, float *values, uint64_t capacity,
                            uint64_t *rows_out);

} // namespace mdb
