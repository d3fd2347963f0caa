// mdb_comoments.hpp - covariance and correlation of two fields (mdb_comoments_buckets*): per date_bin bucket and group
// the count, both means, both m2 and c_xy = the sum of (x - mean_x) * (y - mean_y) over the pairs (x, y) of the bucket.
//
// The first part is plain C++ (no HIP type): a run of pairs accumulated with shifted sums, the merge rule on cells, the
// statistics of a cell and the checks of a request. It is shared by the kernels, by the host entry points
// (mdb_comoments_host.cpp) and by the check program tests/comoments_host, which runs it under the CPU sanitizers. The
// second part (hipcc only) is what one lane makes of one (segment, bucket) pair of the x field.
//
// A run - the pairs of one (segment, bucket) pair, or of one piece inside one bucket - is summed around its first pair
// (Kx, Ky), as mdb_moments.hpp sums a run of one field around its first value:
//   dx = (double)x - Kx   dy = (double)y - Ky   sx += dx   sy += dy   sxx += dx * dx   syy += dy * dy   sxy += dx * dy
//   at the end: means and m2 as moments_finish, c_xy = sxy - sx * sy / n (not clamped: a covariance has a sign).
// Runs are combined by the merge rule only (comoments_merge).
#pragma once

#include "mdb_moments.hpp"

#include <cmath>
#include <limits>

namespace mdb {

// In the call's error word beside the segments' ERR_* bits: a lane asked for a row at or beyond the y column's end.
constexpr uint32_t ERR_COMOMENTS_ROW = 1u << 30;

struct ComomentsRun {
    int64_t n;
    double kx, ky, sx, sy, sxx, syy, sxy;
};

MDB_MOMENTS_FN ComomentsRun comoments_run_empty() { return ComomentsRun{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

MDB_MOMENTS_FN void comoments_point(ComomentsRun &run, float x_value, float y_value) {
    const double x = (double)x_value, y = (double)y_value;
    run.kx = run.n == 0 ? x : run.kx;
    run.ky = run.n == 0 ? y : run.ky;
    const double dx = x - run.kx, dy = y - run.ky;
    run.sx += dx;
    run.sy += dy;
    run.sxx += dx * dx;
    run.syy += dy * dy;
    run.sxy += dx * dy;
    run.n++;
}

// The cell of a run; an empty run gives a fresh cell. Either m2 is clamped at 0 when it rounds below (a comparison,
// not fmax: a NaN stays one); c_xy is not clamped.
MDB_MOMENTS_FN mdb_comoments_cell comoments_finish(const ComomentsRun &run) {
    mdb_comoments_cell cell = {0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (run.n == 0) return cell;
    const double n = (double)run.n;
    double m2_x = run.sxx - run.sx * run.sx / n;
    double m2_y = run.syy - run.sy * run.sy / n;
    if (m2_x < 0.0) m2_x = 0.0;
    if (m2_y < 0.0) m2_y = 0.0;
    cell.count = run.n;
    cell.mean_x = run.kx + run.sx / n;
    cell.mean_y = run.ky + run.sy / n;
    cell.m2_x = m2_x;
    cell.m2_y = m2_y;
    cell.c_xy = run.sxy - run.sx * run.sy / n;
    return cell;
}

// The pairs of `from` added to those of `into`. An empty `from` changes nothing; an empty `into` (count 0: no other
// member is read) takes every member of `from`. The three products are written with one association - that of
// moments_merge's d * d * (na * nb / n) - so identical fields keep m2_x, m2_y and c_xy of the same bytes.
MDB_MOMENTS_FN void comoments_merge(mdb_comoments_cell &into, const mdb_comoments_cell &from) {
    if (from.count == 0) return;
    if (into.count == 0) {
        into = from;
        return;
    }
    const double na = (double)into.count, nb = (double)from.count;
    const int64_t count = into.count + from.count;
    const double n = (double)count;
    const double dx = from.mean_x - into.mean_x, dy = from.mean_y - into.mean_y;
    const double w = na * nb / n;
    into.mean_x = into.mean_x + dx * (nb / n);
    into.mean_y = into.mean_y + dy * (nb / n);
    into.m2_x = into.m2_x + from.m2_x + dx * dx * w;
    into.m2_y = into.m2_y + from.m2_y + dy * dy * w;
    into.c_xy = into.c_xy + from.c_xy + dx * dy * w;
    into.count = count;
}

// The statistic `kind` (MDB_COMOMENTS_*, checked by the caller) of a cell; x is the independent variable.
inline double comoments_statistic(const mdb_comoments_cell &cell, uint32_t kind) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int64_t count = cell.count;
    if (count == 0) return nan;
    const double n = (double)count;
    if (kind == MDB_COMOMENTS_COVAR_POP) return cell.c_xy / n;
    if (count <= 1) return nan;
    if (kind == MDB_COMOMENTS_COVAR_SAMP) return cell.c_xy / (n - 1.0);
    if (kind == MDB_COMOMENTS_CORR || kind == MDB_COMOMENTS_REGR_R2) {
        if (cell.m2_x == 0.0 || cell.m2_y == 0.0) return nan;
        if (kind == MDB_COMOMENTS_CORR) return cell.c_xy / std::sqrt(cell.m2_x * cell.m2_y);
        return cell.c_xy * cell.c_xy / (cell.m2_x * cell.m2_y);
    }
    if (cell.m2_x == 0.0) return nan;
    const double slope = cell.c_xy / cell.m2_x;
    return kind == MDB_COMOMENTS_REGR_SLOPE ? slope : cell.mean_y - slope * cell.mean_x;
}

// The host-side checks every form makes before it touches the device: those of mdb_moments_buckets*.
inline int comoments_request_check(const mdb_bucket_request *request, uint64_t *n_cells) {
    if (request->which_mask != 0) return fail("which_mask must be 0 for mdb_comoments_buckets*.");
    if (request->width <= 0) return fail("The bucket width must be positive.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    const unsigned __int128 cells = (unsigned __int128)request->n_groups * request->n_buckets;
    if (cells * sizeof(mdb_comoments_cell) > (unsigned __int128)UINT64_MAX) return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// mdb_comoments.hip: the host batches of the two lists uploaded (a batch that is in both lists once) and folded into
// the caller's cells (the request checked, xs not empty). The only step of the host forms that needs the device.
int comoments_list_run(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                       uint32_t n_y, const uint32_t *const *group_of_segment_x, const mdb_bucket_request *request,
                       uint64_t n_cells, mdb_comoments_cell *inout);

} // namespace mdb

#if defined(__HIPCC__)

namespace mdb {

__device__ __forceinline__ mdb_comoments_cell comoments_empty() { return mdb_comoments_cell{0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// What the tree and fold (mdb_bucket_fold.hpp) need to know of a comoments cell: for mdb_comoments.hip and for
// mdb_trend.hip, whose partials are comoments cells too (each instantiates BucketFold<ComomentsFoldOps> itself).
struct ComomentsFoldOps : FoldOps<mdb_comoments_cell> {
    static constexpr const char *tree_name = "k_comoments_tree", *fold_name = "k_comoments_fold";
    __device__ __forceinline__ static mdb_comoments_cell empty() { return comoments_empty(); }
    __device__ __forceinline__ static void merge(mdb_comoments_cell &into, const mdb_comoments_cell &from) { comoments_merge(into, from); }
    __device__ __forceinline__ static bool is_empty(const mdb_comoments_cell &acc) { return acc.count == 0; }
    __device__ __forceinline__ void apply(mdb_comoments_cell &cell, const mdb_comoments_cell &acc) const { comoments_merge(cell, acc); }
};

// The y column: one f32 per row of the range grid of the y field. The row of point k of an x segment is `base` + k,
// where base = the segment's first row - the index of its first point inside [t_lo, t_hi] (wrapping arithmetic: the
// sum is exact). Two batches that line up never ask for a row at or beyond n_rows: the row arithmetic here and the
// range grid's would have to disagree. Such a row is not read; it raises ERR_COMOMENTS_ROW, so the call fails.
struct YColumn {
    const float *values;
    uint64_t n_rows;
    __device__ __forceinline__ float at(uint64_t row, uint32_t *error) const {
        if (row < n_rows) return values[row];
        *error |= ERR_COMOMENTS_ROW;
        return __uint_as_float(0x7fc00000u);
    }
};

// mdb_comoments.hip (mdb_binned.hip too): the rows of x and y under [t_lo, t_hi] compared - a mismatch fails with both
// counts - x's first rows (n + 1 of them, SCRATCH_COMOMENTS_ROWS) and the y column (SCRATCH_COMOMENTS_YCOL). Both slots
// are filled anew by every call that reads them, under the context's lock.
int comoments_rows(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, int64_t t_lo, int64_t t_hi,
                   const unsigned long long **first_row, YColumn *column);

// The model points [a, b] of a PMC-Mean or Swing segment with regular timestamps as one run, point by point in
// registers on the x side (as moments_model_points does for Swing), one read of the y column per point: there is no
// O(1) case, not for PMC-Mean either - the y side needs every row.
__device__ __forceinline__ void comoments_model_points(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b,
                                                       uint64_t row_base, const YColumn &y, uint32_t *error,
                                                       mdb_comoments_cell &acc) {
    ComomentsRun run = comoments_run_empty();
    int64_t t = d.start + (int64_t)((uint64_t)a * (uint64_t)d.delta);
    for (uint32_t index = a;; index++) {
        comoments_point(run, model_value_at(d, type, t), y.at(row_base + index, error));
        if (index == b) break;
        t = (int64_t)((uint64_t)t + (uint64_t)d.delta);
    }
    comoments_merge(acc, comoments_finish(run));
}

// The points of a PMC-Mean or Swing segment with regular timestamps inside [lo, hi]: the model's as above, the
// residual tail's decoded as a run of its own (not when the tail is k_comoments_pieces').
__device__ __forceinline__ mdb_comoments_cell comoments_regular_pair(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                                     int64_t lo, int64_t hi, uint64_t row_base,
                                                                     const YColumn &y, uint32_t *error,
                                                                     bool tail_by_pieces) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const uint32_t n_res = d.n_total - d.n_model;
    mdb_comoments_cell acc = comoments_empty();
    uint32_t k_lo = 0, k_hi = 0;
    if (!regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi)) return acc;
    if (k_lo < d.n_model) comoments_model_points(d, type, k_lo, min(k_hi, d.n_model - 1), row_base, y, error, acc);
    if (n_res > 0 && k_hi >= d.n_model && !tail_by_pieces) {
        const uint4 vr = s.residuals.views[i];
        ComomentsRun run = comoments_run_empty();
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, k_hi - d.n_model + 1, true, __float_as_uint(d.value),
                         error, [&](uint32_t k, uint32_t bits) {
                             if (d.n_model + k >= k_lo)
                                 comoments_point(run, __uint_as_float(bits), y.at(row_base + d.n_model + k, error));
                         });
        comoments_merge(acc, comoments_finish(run));
    }
    return acc;
}

// Where pass 1 of a stream leaves slot j's index interval [x, y] of points (x > y: none): the cell's first 8 bytes.
// (Copied as bytes: the slot is read and written as a cell too.)
__device__ __forceinline__ uint2 comoments_interval(const mdb_comoments_cell *slot) {
    uint2 interval;
    __builtin_memcpy(&interval, slot, 8);
    return interval;
}
__device__ __forceinline__ void comoments_set_interval(mdb_comoments_cell *slot, uint32_t k_lo, uint32_t k_hi) {
    const uint2 interval = make_uint2(k_lo, k_hi);
    __builtin_memcpy(slot, &interval, 8);
}

// Pass 2 over the slots [j0, j1) of a segment whose points are a bit stream, each slot holding its index interval
// (ascending, disjoint): the values are decoded once, up to point `needed` - 1, each with its row of the y column
// into the run of the slot whose interval holds it, and every slot is overwritten with the cell of its run
// (moments_stream_decode with a second value per point).
__device__ __forceinline__ void comoments_stream_decode(const DevSegments &s, uint64_t i, const SegInfo &info, uint64_t j0,
                                                        uint64_t j1, uint64_t p0, mdb_comoments_cell *__restrict__ out,
                                                        uint32_t needed, uint64_t row_base, const YColumn &y,
                                                        uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint32_t n_res = d.n_total - d.n_model;
    uint64_t j = j0;
    uint2 current = comoments_interval(&out[j - p0]);
    ComomentsRun run = comoments_run_empty();
    auto flush = [&]() {
        out[j - p0] = comoments_finish(run);
        run = comoments_run_empty();
        j++;
        if (j < j1) current = comoments_interval(&out[j - p0]);
    };
    auto visit = [&](uint32_t k, float v) {
        while (j < j1 && k > current.y) flush();
        if (j < j1 && k >= current.x) comoments_point(run, v, y.at(row_base + k, error));
    };
    if (needed > 0) {
        float seed = d.value;
        if (type == MDB_MACAQUE_V_ID) {
            const uint4 vv = s.values.views[i];
            uint32_t last_bits = 0;
            const bool residuals_needed = n_res > 0 && needed > d.n_model;
            decode_macaque_v(view_data(s.values, i, vv), vv.x, residuals_needed ? d.n_model : min(d.n_model, needed),
                             false, 0, error, [&](uint32_t k, uint32_t bits) {
                                 visit(k, __uint_as_float(bits));
                                 last_bits = bits;
                             });
            seed = __uint_as_float(last_bits);
        } else if (d.n_model > 0) { // PMC-Mean / Swing on irregular timestamps: the model at each timestamp
            const uint4 vt = s.timestamps.views[i];
            decode_irregular_timestamps(view_data(s.timestamps, i, vt), vt.x, d.start, end, min(d.n_model, needed), error,
                                        [&](uint32_t k, int64_t t) {
                                            if (k < d.n_model) visit(k, model_value_at(d, type, t));
                                        });
        }
        if (n_res > 0 && needed > d.n_model) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, needed - d.n_model, true, __float_as_uint(seed),
                             error, [&](uint32_t k, uint32_t bits) { visit(d.n_model + k, __uint_as_float(bits)); });
        }
    }
    while (j < j1) flush();
}

// The pairs of a segment whose points are a bit stream (MacaqueV values, irregular timestamps): slots [j0, j1) of the
// slice, buckets b_first + (j - off), as moments_stream_partials - pass 1 leaves each slot's index interval and finds
// the index of the segment's first point inside [t_lo, t_hi] (row 0 of the segment), comoments_stream_decode does the
// rest. Returns false when the timestamps turn out not to be sorted (a malformed stream): the caller then goes pair
// by pair (comoments_unsorted_pair).
__device__ __forceinline__ bool comoments_stream_partials(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                          const BucketRequest &r, uint64_t off, uint64_t b_first,
                                                          uint64_t j0, uint64_t j1, uint64_t p0,
                                                          mdb_comoments_cell *__restrict__ out, uint64_t first_row,
                                                          const YColumn &y, uint32_t *error) {
    const SegDesc &d = info.desc;
    const int64_t end = s.end_time[i];
    uint32_t needed = 0;  // points [0, needed) reach a slot
    uint32_t k_first = 0; // the first point inside [t_lo, t_hi]
    if (d.flags & FLAG_REGULAR) {
        uint32_t k_last = 0;
        (void)regular_index_interval(d.start, d.delta, d.n_total, r.t_lo, r.t_hi, &k_first, &k_last);
        for (uint64_t j = j0; j < j1; j++) {
            int64_t lo, hi;
            bucket_bounds(r, b_first + (j - off), &lo, &hi);
            uint32_t k_lo = 1, k_hi = 0;
            if (regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi)) needed = k_hi + 1;
            else k_lo = 1, k_hi = 0;
            comoments_set_interval(&out[j - p0], k_lo, k_hi);
        }
    } else {
        for (uint64_t j = j0; j < j1; j++) comoments_set_interval(&out[j - p0], 1, 0);
        const uint4 vt = s.timestamps.views[i];
        uint64_t slot = ~0ull;
        uint32_t k_lo = 0, k_hi = 0;
        int64_t previous = INT64_MIN;
        bool sorted = true, any_in_range = false;
        decode_irregular_timestamps(view_data(s.timestamps, i, vt), vt.x, d.start, end, 0xffffffffu, error,
                                    [&](uint32_t k, int64_t t) {
                                        if (t < previous) sorted = false;
                                        previous = t;
                                        if (!sorted || t < r.t_lo || t > r.t_hi) return;
                                        if (!any_in_range) {
                                            any_in_range = true;
                                            k_first = k;
                                        }
                                        if (t < r.origin) return;
                                        const uint64_t b = ((uint64_t)t - (uint64_t)r.origin) / (uint64_t)r.width;
                                        if (b < b_first || b >= r.n_buckets) return;
                                        const uint64_t j = off + (b - b_first);
                                        if (j < j0 || j >= j1) return;
                                        if (j != slot) {
                                            if (slot != ~0ull) comoments_set_interval(&out[slot - p0], k_lo, k_hi);
                                            slot = j;
                                            k_lo = k;
                                        }
                                        k_hi = k;
                                    });
        if (!sorted) return false;
        if (slot != ~0ull) {
            comoments_set_interval(&out[slot - p0], k_lo, k_hi);
            needed = k_hi + 1;
        }
    }
    comoments_stream_decode(s, i, info, j0, j1, p0, out, needed, first_row - k_first, y, error);
    return true;
}

// One pair [lo, hi] of a segment with irregular timestamps that are not sorted (a malformed stream), into *slot: the
// points the range aggregate counts for the same bounds, as moments_unsorted_pair, with the rows segment_range
// (mdb_agg_dev.hpp) gives them under [t_lo, t_hi]. A model without residuals: every point is tested with its own
// timestamp, its row the running count of the points inside [t_lo, t_hi]. Values in a bit stream: the indices
// between the first and the last timestamp inside [lo, hi], point k at row k - the first index inside [t_lo, t_hi].
__device__ __forceinline__ void comoments_unsorted_pair(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                        const BucketRequest &r, int64_t lo, int64_t hi, uint64_t j,
                                                        uint64_t p0, mdb_comoments_cell *__restrict__ out,
                                                        uint64_t first_row, const YColumn &y, uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint4 vt = s.timestamps.views[i];
    const uint8_t *ts_bytes = view_data(s.timestamps, i, vt);
    if (type != MDB_MACAQUE_V_ID && d.n_total == d.n_model) {
        ComomentsRun run = comoments_run_empty();
        if (!(end < lo || d.start > hi)) {
            uint64_t row = first_row;
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t, int64_t t) {
                if (t < r.t_lo || t > r.t_hi) return;
                if (t >= lo && t <= hi) comoments_point(run, model_value_at(d, type, t), y.at(row, error));
                row += 1;
            });
        }
        out[j - p0] = comoments_finish(run);
        return;
    }
    uint32_t k_lo = 0xffffffffu, k_hi = 0, k_first = 0xffffffffu;
    if (!(end < lo || d.start > hi))
        decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t k, int64_t t) {
            if (t >= r.t_lo && t <= r.t_hi && k < k_first) k_first = k;
            if (t >= lo && t <= hi) {
                if (k < k_lo) k_lo = k;
                if (k > k_hi) k_hi = k;
            }
        });
    const bool any = k_lo != 0xffffffffu; // (then k_first is set as well: [lo, hi] lies inside [t_lo, t_hi])
    comoments_set_interval(&out[j - p0], any ? k_lo : 1u, any ? k_hi : 0u);
    comoments_stream_decode(s, i, info, j, j + 1, p0, out, any ? k_hi + 1 : 0, first_row - (any ? k_first : 0u), y, error);
}

} // namespace mdb

#endif // __HIPCC__
