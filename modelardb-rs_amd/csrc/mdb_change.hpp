// mdb_change.hpp - changes between consecutive points per date_bin bucket (mdb_change_buckets*): the series as a
// sequence of steps. Per bucket and group one mdb_change_cell over the LINKED pairs of rows (mdb.h: the rule of
// mdb_integral_buckets, integral_linked) whose LATER row lies in the bucket; a pair is never cut.
//
// The first part is plain C++ (no HIP type): the arithmetic of one pair, the accumulator of a cell, the merge, the
// walk of a run of points, the closed form of PMC-Mean rows on regular timestamps and the request's checks. It is
// shared by the kernels, by the host entry points (mdb_change_host.cpp) and by the check program tests/change_host,
// which runs it under the CPU sanitizers. The second part (hipcc only) is what one lane makes of one segment.
//
// Arithmetic. A step is d = (double)v1 - (double)v0: both conversions are exact, the subtraction rounds once. A time
// difference is formed in uint64_t (below 2^64 for any two int64 instants). The bucket of an instant t >= origin is
// (t - origin) / width in uint64_t; a bucket's first instant is formed wrapping (exact for a bucket a real timestamp
// reaches) and its last instant saturates at INT64_MAX.
#pragma once

#include "mdb_integral.hpp"

namespace mdb {

MDB_INTEGRAL_FN mdb_change_cell change_cell_empty() { return mdb_change_cell{0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// The linked pair (t0, v0) - (t1, v1), t1 > t0, added to the cell of t1's bucket.
MDB_INTEGRAL_FN void change_cell_pair(mdb_change_cell &cell, int64_t t0, float v0, int64_t t1, float v1) {
    const double d = (double)v1 - (double)v0;
    cell.count += 1;
    cell.duration += (uint64_t)t1 - (uint64_t)t0;
    if (d > 0.0) {
        cell.rise += d;
        if (d > cell.max_rise) cell.max_rise = d;
    } else if (d < 0.0) {
        cell.n_fall += 1;
        cell.fall += -d;
        cell.reset_sum += (double)v1;
        if (-d > cell.max_fall) cell.max_fall = -d;
    } else if (d != d) { // a NaN value, or inf - inf: the two sums say so, the counts stay exact
        cell.rise += d;
        cell.fall += d;
    }
}

// `pairs` linked pairs of one value v, `delta` microseconds apart each (PMC-Mean rows): d is v - v, which is 0 or NaN.
MDB_INTEGRAL_FN void change_cell_constant_pairs(mdb_change_cell &cell, uint64_t pairs, uint64_t delta, float v) {
    if (pairs == 0) return;
    cell.count += pairs;
    cell.duration += pairs * delta;
    const double d = (double)v - (double)v;
    if (d != d) {
        cell.rise += d;
        cell.fall += d;
    }
}

MDB_INTEGRAL_FN void change_cell_merge(mdb_change_cell &into, const mdb_change_cell &from) {
    into.count += from.count;
    into.n_fall += from.n_fall;
    into.duration += from.duration;
    into.rise += from.rise;
    into.fall += from.fall;
    into.reset_sum += from.reset_sum;
    if (from.max_rise > into.max_rise) into.max_rise = from.max_rise;
    if (from.max_fall > into.max_fall) into.max_fall = from.max_fall;
}

// The last instant of the bucket that starts at `start`, saturating at INT64_MAX.
MDB_INTEGRAL_FN int64_t change_bucket_last(int64_t start, int64_t width) {
    const uint64_t room = (uint64_t)INT64_MAX - (uint64_t)start;
    return (uint64_t)width - 1 > room ? INT64_MAX : (int64_t)((uint64_t)start + ((uint64_t)width - 1));
}

// The rows k in [1, n) of the points start + k * delta, delta > 0, with lo <= start + k * delta <= hi: the LATER rows
// of the pairs (k - 1, k) that belong to [lo, hi]. Returns how many, [*ka, *kb] when there are any. O(1).
MDB_INTEGRAL_FN uint64_t change_regular_rows(int64_t start, int64_t delta, uint32_t n, int64_t lo, int64_t hi,
                                             uint32_t *ka, uint32_t *kb) {
    if (n < 2 || delta <= 0 || hi <= start || lo > hi) return 0;
    const uint64_t step = (uint64_t)delta;
    const int64_t last = (int64_t)((uint64_t)start + (uint64_t)(n - 1) * step);
    if (lo > last) return 0;
    uint64_t a = 1;
    if (lo > start) {
        const uint64_t from = (uint64_t)lo - (uint64_t)start;
        a = from / step + (from % step != 0); // (>= 1; <= n - 1 as lo <= last)
    }
    const uint64_t b = hi >= last ? (uint64_t)(n - 1) : ((uint64_t)hi - (uint64_t)start) / step;
    if (b < a) return 0;
    *ka = (uint32_t)a;
    *kb = (uint32_t)b;
    return b - a + 1;
}

// The buckets [b0, b1) a walk may write, cells[b - b0]. A pair whose later row lies outside the window is dropped.
struct ChangeWindow {
    int64_t origin, width, max_gap;
    uint64_t b0, b1;
    mdb_change_cell *cells;
};

// A run of rows of one group, fed point by point in row order: every linked pair is added to the cell of its later
// row's bucket - the cell of the bucket at hand is held in registers and MERGED into the window's when the walk moves
// to another bucket (in either direction: a malformed stream may step back in time) or ends.
struct ChangeWalk {
    mdb_change_cell acc;
    uint64_t bucket;
    int64_t lo, hi; // the first and the last instant of the open bucket: a row between them needs no division
    int64_t t_prev;
    float v_prev;
    bool open, have;
};

MDB_INTEGRAL_FN ChangeWalk change_walk_start() { return ChangeWalk{change_cell_empty(), 0, 0, 0, 0, 0.0f, false, false}; }

MDB_INTEGRAL_FN void change_walk_flush(const ChangeWindow &w, ChangeWalk &walk) {
    if (walk.open) change_cell_merge(w.cells[walk.bucket - w.b0], walk.acc);
    walk.open = false;
    walk.acc = change_cell_empty();
}

MDB_INTEGRAL_FN void change_walk_point(const ChangeWindow &w, ChangeWalk &walk, int64_t t, float v) {
    if (walk.have && integral_linked(w.max_gap, walk.t_prev, t)) {
        if (walk.open && t >= walk.lo && t <= walk.hi) {
            change_cell_pair(walk.acc, walk.t_prev, walk.v_prev, t, v);
        } else if (walk.open && t > walk.hi && (uint64_t)t - (uint64_t)walk.hi <= (uint64_t)w.width &&
                   walk.bucket + 1 < w.b1) { // the next bucket (hi < t <= INT64_MAX: hi + 1 does not overflow)
            change_walk_flush(w, walk);
            walk.open = true;
            walk.bucket += 1;
            walk.lo = walk.hi + 1;
            walk.hi = change_bucket_last(walk.lo, w.width);
            change_cell_pair(walk.acc, walk.t_prev, walk.v_prev, t, v);
        } else if (t >= w.origin) {
            const uint64_t b = ((uint64_t)t - (uint64_t)w.origin) / (uint64_t)w.width;
            if (b >= w.b0 && b < w.b1) {
                change_walk_flush(w, walk);
                walk.open = true;
                walk.bucket = b;
                walk.lo = integral_bucket_start(w.origin, w.width, b); // (<= t, a real timestamp: exact)
                walk.hi = change_bucket_last(walk.lo, w.width);
                change_cell_pair(walk.acc, walk.t_prev, walk.v_prev, t, v);
            }
        }
    }
    walk.have = true;
    walk.t_prev = t;
    walk.v_prev = v;
}

// The host-side checks every form makes before it touches the device.
inline int change_request_check(const mdb_change_request *request, uint64_t *n_cells) {
    const mdb_bucket_request &b = request->buckets;
    if (b.which_mask != 0) return fail("which_mask must be 0 for mdb_change_buckets*.");
    if (b.width <= 0) return fail("The bucket width must be positive.");
    if (b.n_groups == 0) return fail("n_groups must be at least 1.");
    if (b.t_lo != INT64_MIN || b.t_hi != INT64_MAX)
        return fail("mdb_change_buckets* takes no time range: t_lo / t_hi must be INT64_MIN / INT64_MAX.");
    if (request->reserved != 0) return fail("mdb_change_request.reserved must be 0.");
    if (request->flags != 0) return fail("mdb_change_request.flags must be 0.");
    if (request->max_gap < 0) return fail("max_gap must not be negative.");
    const unsigned __int128 cells = (unsigned __int128)b.n_groups * b.n_buckets;
    if (cells * sizeof(mdb_change_cell) > (unsigned __int128)UINT64_MAX) return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// mdb_change.hip: the host batches of the list uploaded and folded into the caller's cells (the request checked, the
// list not empty). The only step of the host forms that needs the device.
int change_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                    uint32_t n_inputs, const mdb_change_request *request, uint64_t n_cells, mdb_change_cell *inout);

} // namespace mdb

#if defined(__HIPCC__)

namespace mdb {

// Slots [j0, j1) of the slice (slot j: bucket b_first + (j - off)) for segment i, whose pair with its right
// neighbour's first row (same group; `heads`) is the segment's own. PMC-Mean rows on regular timestamps: count and
// duration per slot from row indices, O(1), no loop over rows. Swing rows on regular timestamps: the rows of the
// slots' window one by one in registers, no memory touched. Then only the residual tail and the link are walked,
// behind the model's last point. Everything else - MacaqueV values, irregular timestamps - is one walk of the rows.
__device__ __forceinline__ void change_segment_partials(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                        const IntegralRequest &q, uint64_t off, uint64_t b_first,
                                                        uint64_t j0, uint64_t j1, uint64_t p0,
                                                        mdb_change_cell *__restrict__ out, bool neighbour,
                                                        const IntegralHead *__restrict__ heads, uint32_t *error) {
    const SegDesc &d = info.desc;
    const BucketRequest &r = q.buckets;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const bool regular = (d.flags & FLAG_REGULAR) != 0;
    const ChangeWindow w = {r.origin, r.width, q.max_gap, b_first + (j0 - off), b_first + (j1 - off), out + (j0 - p0)};
    const bool model = regular && type != MDB_MACAQUE_V_ID && d.n_model >= 1;
    const bool closed = model && d.n_model >= 2 && integral_linked(q.max_gap, 0, d.delta);
    const bool constant = type == MDB_PMC_MEAN_ID;
    for (uint64_t j = j0; j < j1; j++) {
        mdb_change_cell cell = change_cell_empty();
        if (closed && constant) {
            const int64_t start = integral_bucket_start(r.origin, r.width, b_first + (j - off));
            uint32_t ka = 0, kb = 0;
            const uint64_t pairs =
                change_regular_rows(d.start, d.delta, d.n_model, start, change_bucket_last(start, r.width), &ka, &kb);
            change_cell_constant_pairs(cell, pairs, (uint64_t)d.delta, d.value);
        }
        out[j - p0] = cell;
    }
    const int64_t window_last = change_bucket_last(integral_bucket_start(r.origin, r.width, w.b1 - 1), r.width);
    const IntegralHead head = neighbour ? heads[i + 1] : IntegralHead{0.0f, 0u};
    const int64_t next = neighbour ? s.start_time[i + 1] : 0;
    const int64_t t_last = regular ? (d.n_total > 0 ? trend_time_at(d, d.n_total - 1) : d.start) : s.end_time[i];
    const bool link = neighbour && head.rows > 0 && d.n_total > 0 && integral_linked(q.max_gap, t_last, next);
    ChangeWalk walk = change_walk_start();
    const uint32_t n_res = d.n_total - d.n_model;
    if (model) {
        if (closed && !constant) { // Swing: the later rows inside the window, each against the row before it
            const int64_t window_first = integral_bucket_start(r.origin, r.width, w.b0);
            uint32_t ka = 0, kb = 0;
            if (change_regular_rows(d.start, d.delta, d.n_model, window_first, window_last, &ka, &kb)) {
                for (uint32_t k = ka - 1; k <= kb; k++) {
                    const int64_t t = trend_time_at(d, k);
                    change_walk_point(w, walk, t, model_value_at(d, type, t));
                }
            }
        }
        if (n_res > 0 || link) change_walk_point(w, walk, trend_time_at(d, d.n_model - 1), d.value);
        if (n_res > 0) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, n_res, true, __float_as_uint(d.value), error,
                             [&](uint32_t k, uint32_t bits) {
                                 change_walk_point(w, walk, trend_time_at(d, d.n_model + k), __uint_as_float(bits));
                             });
        }
    } else {
        // How far the rows are needed on regular timestamps: to the end when the link wants the last value, else to
        // the last row inside the window.
        uint32_t limit = d.n_total;
        if (regular && !link && d.delta > 0 && d.n_total > 0) {
            if (window_last <= d.start) limit = 1;
            else if (window_last < t_last)
                limit = (uint32_t)min((uint64_t)d.n_total, ((uint64_t)window_last - (uint64_t)d.start) / (uint64_t)d.delta + 1);
        }
        integral_rows(s, i, info, limit, error, [&](int64_t t, float v) { change_walk_point(w, walk, t, v); });
    }
    if (link) change_walk_point(w, walk, next, head.value);
    change_walk_flush(w, walk);
}

} // namespace mdb

#endif // __HIPCC__
