// mdb_integral.hpp - time-weighted averages and integrals per date_bin bucket (mdb_integral_buckets*): the series as a
// function of time. Per bucket and group one mdb_integral_cell {duration, integral} over the LINKED intervals of the
// rows (mdb.h: same group, time moving forward, the gap within max_gap), clipped to the bucket.
//
// The first part is plain C++ (no HIP type): the linked rule, the bucket edges, the integral of one clipped piece, the
// accumulator of a cell, the walk of a run of points over the buckets it crosses, the closed form of a model on
// regular timestamps and the request's checks. It is shared by the kernels, by the host entry points
// (mdb_integral_host.cpp) and by the check program tests/integral_host, which runs it under the CPU sanitizers. The
// second part (hipcc only) is what one lane makes of one segment.
//
// Arithmetic. Every time difference is formed in uint64_t (it is below 2^64 for any two int64 instants) and converted
// to f64 once. A bucket's first instant origin + b * width is formed wrapping; for a bucket a real timestamp reaches it
// is exact. Its end saturates at INT64_MAX, which no piece notices: a piece ends at min(t1, end). A piece on which the
// function is constant (STEP always, LINEAR when v0 == v1) is not multiplied out at once: equal neighbours are joined
// into a run of integer length, multiplied once (IntegralAcc). A constant stretch of any number of points then
// carries one rounding, which is what keeps a constant cell's average within 2^-44 of its level.
#pragma once

#if defined(__HIPCC__)
#include "mdb_trend.hpp"
#define MDB_INTEGRAL_FN __host__ __device__ __forceinline__
#else
#include "mdb_host_side.hpp"
#define MDB_INTEGRAL_FN inline
#endif

#include <cstdint>

namespace mdb {

// Is the row at t linked to its predecessor at t_prev (the groups are the caller's to compare)? The difference is
// formed after the comparison, in uint64_t: it cannot overflow.
MDB_INTEGRAL_FN bool integral_linked(int64_t max_gap, int64_t t_prev, int64_t t) {
    return t > t_prev && (uint64_t)t - (uint64_t)t_prev <= (uint64_t)max_gap;
}

MDB_INTEGRAL_FN int64_t integral_bucket_start(int64_t origin, int64_t width, uint64_t b) {
    return (int64_t)((uint64_t)origin + b * (uint64_t)width);
}
// The (exclusive) end of the bucket that starts at `start`, saturating at INT64_MAX.
MDB_INTEGRAL_FN int64_t integral_bucket_end(int64_t start, int64_t width) {
    const uint64_t room = (uint64_t)INT64_MAX - (uint64_t)start;
    return (uint64_t)width > room ? INT64_MAX : (int64_t)((uint64_t)start + (uint64_t)width);
}

// The integral of f over [a, e] inside the linked interval [t0, t1] with t0 <= a < e <= t1 and v0 != v1, LINEAR:
// the length times f at the piece's middle, the middle as a fraction of the interval.
MDB_INTEGRAL_FN double integral_linear_piece(int64_t t0, float v0, int64_t t1, float v1, int64_t a, int64_t e) {
    const double length = (double)((uint64_t)e - (uint64_t)a);
    const double whole = (double)((uint64_t)t1 - (uint64_t)t0);
    const double from = (double)((uint64_t)a - (uint64_t)t0), to = (double)((uint64_t)e - (uint64_t)t0);
    const double middle = (from + to) * 0.5 / whole;
    return length * ((double)v0 + ((double)v1 - (double)v0) * middle);
}

// What a lane holds of one cell: the pieces so far, and the open run of pieces of one level.
struct IntegralAcc {
    uint64_t duration;
    double integral;
    uint64_t run; // microseconds at `level` not yet multiplied out
    float level;
};

MDB_INTEGRAL_FN IntegralAcc integral_acc_empty() { return IntegralAcc{0, 0.0, 0, 0.0f}; }

MDB_INTEGRAL_FN void integral_acc_close(IntegralAcc &acc) {
    if (acc.run) acc.integral += (double)acc.run * (double)acc.level;
    acc.run = 0;
}

MDB_INTEGRAL_FN void integral_acc_constant(IntegralAcc &acc, uint64_t length, float level) {
    if (acc.run && !(level == acc.level)) integral_acc_close(acc); // (a NaN never joins a run: each piece is its own)
    acc.level = level;
    acc.run += length;
    acc.duration += length;
}

// The piece [a, e] of the linked interval (t0, v0) - (t1, v1).
MDB_INTEGRAL_FN void integral_acc_piece(IntegralAcc &acc, uint32_t method, int64_t t0, float v0, int64_t t1, float v1,
                                        int64_t a, int64_t e) {
    const uint64_t length = (uint64_t)e - (uint64_t)a;
    if (method == MDB_INTEGRAL_STEP || v0 == v1) {
        integral_acc_constant(acc, length, v0);
    } else {
        acc.duration += length;
        acc.integral += integral_linear_piece(t0, v0, t1, v1, a, e);
    }
}

MDB_INTEGRAL_FN mdb_integral_cell integral_acc_cell(IntegralAcc acc) {
    integral_acc_close(acc);
    return mdb_integral_cell{acc.duration, acc.integral};
}

MDB_INTEGRAL_FN void integral_cell_add(mdb_integral_cell &into, const mdb_integral_cell &from) {
    into.duration += from.duration;
    into.integral += from.integral;
}

// The buckets [b0, b1) a walk may write, cells[b - b0]: those of b0 .. b1 - 1 are reached by a real timestamp (the
// span's promise), so their first instants are exact. What a walk finds outside the window is dropped.
struct IntegralWindow {
    int64_t origin, width, max_gap;
    uint64_t b0, b1;
    uint32_t method;
    mdb_integral_cell *cells;
};

// A run of rows of one group, fed point by point in row order: every linked interval is cut at the bucket edges it
// crosses and its pieces are ADDED to the window's cells - the cell of the bucket at hand is held in registers and
// written when the walk moves to another bucket (in either direction: a malformed stream may step back in time, which
// links nothing but may land in an earlier bucket) or ends.
struct IntegralWalk {
    IntegralAcc acc;
    uint64_t bucket;
    int64_t t_prev;
    float v_prev;
    bool open, have;
};

MDB_INTEGRAL_FN IntegralWalk integral_walk_start() {
    return IntegralWalk{integral_acc_empty(), 0, 0, 0.0f, false, false};
}

MDB_INTEGRAL_FN void integral_walk_flush(const IntegralWindow &w, IntegralWalk &walk) {
    if (walk.open) integral_cell_add(w.cells[walk.bucket - w.b0], integral_acc_cell(walk.acc));
    walk.open = false;
    walk.acc = integral_acc_empty();
}

// The linked interval (t0, v0) - (t1, v1), t1 > t0, over the window's buckets.
MDB_INTEGRAL_FN void integral_walk_interval(const IntegralWindow &w, IntegralWalk &walk, int64_t t0, float v0,
                                            int64_t t1, float v1) {
    if (w.b0 >= w.b1) return;
    const int64_t window_start = integral_bucket_start(w.origin, w.width, w.b0);
    const int64_t from = t0 > window_start ? t0 : window_start;
    if (t1 <= from) return;
    uint64_t b = ((uint64_t)from - (uint64_t)w.origin) / (uint64_t)w.width; // (from >= window_start >= origin)
    while (b < w.b1) {
        const int64_t start = integral_bucket_start(w.origin, w.width, b); // (<= from < t1: exact)
        const int64_t end = integral_bucket_end(start, w.width);
        const int64_t a = t0 > start ? t0 : start, e = t1 < end ? t1 : end;
        if (e <= a) break;
        if (!walk.open || walk.bucket != b) {
            integral_walk_flush(w, walk);
            walk.open = true;
            walk.bucket = b;
        }
        integral_acc_piece(walk.acc, w.method, t0, v0, t1, v1, a, e);
        if (t1 <= end) break;
        b++;
    }
}

// The next row of the run.
MDB_INTEGRAL_FN void integral_walk_point(const IntegralWindow &w, IntegralWalk &walk, int64_t t, float v) {
    if (walk.have && integral_linked(w.max_gap, walk.t_prev, t)) integral_walk_interval(w, walk, walk.t_prev, walk.v_prev, t, v);
    walk.have = true;
    walk.t_prev = t;
    walk.v_prev = v;
}

// The share of bucket [bucket_start, bucket_end) in the points k in [0, n) at start + k * delta, delta > 0, every two
// neighbours linked - a model on regular timestamps - in O(1): value_at(k) is point k's value, sum_of(a, b) the f64
// sum of the values of points a .. b (mdb_agg_dev.hpp's model_closed_form on the device: its cancellation guard and
// its pointwise fallback apply). `constant`: every value is value_at(0) (PMC-Mean): value x clipped duration.
// Otherwise (Swing) the whole intervals [ka, kb] inside the bucket are, with neighbours delta apart,
//   LINEAR  delta * (sum(ka .. kb) - (v_ka + v_kb) / 2)        STEP  delta * sum(ka .. kb - 1)
// and the two intervals the bucket's edges cut are pieces of their own, each from its two point values. A bucket that
// lies inside one interval is one piece.
template <typename ValueAt, typename SumOf>
MDB_INTEGRAL_FN mdb_integral_cell integral_regular_cell(uint32_t method, int64_t start, int64_t delta, uint32_t n,
                                                        int64_t bucket_start, int64_t bucket_end, bool constant,
                                                        ValueAt value_at, SumOf sum_of) {
    mdb_integral_cell cell = {0, 0.0};
    if (n < 2) return cell;
    const int64_t last = (int64_t)((uint64_t)start + (uint64_t)(n - 1) * (uint64_t)delta);
    const int64_t a = start > bucket_start ? start : bucket_start, e = last < bucket_end ? last : bucket_end;
    if (e <= a) return cell;
    cell.duration = (uint64_t)e - (uint64_t)a;
    if (constant) {
        cell.integral = (double)cell.duration * (double)value_at(0u);
        return cell;
    }
    const uint64_t step = (uint64_t)delta, from = (uint64_t)a - (uint64_t)start, to = (uint64_t)e - (uint64_t)start;
    const uint32_t ka = (uint32_t)(from / step + (from % step != 0)); // the first point at or behind a (<= n - 1)
    const uint32_t kb = (uint32_t)(to / step);                        // the last point at or before e
    auto time_at = [&](uint32_t k) { return (int64_t)((uint64_t)start + (uint64_t)k * step); };
    IntegralAcc acc = integral_acc_empty();
    if (kb < ka) { // (kb == ka - 1: the bucket lies inside one interval)
        integral_acc_piece(acc, method, time_at(kb), value_at(kb), time_at(ka), value_at(ka), a, e);
        cell.integral = integral_acc_cell(acc).integral;
        return cell;
    }
    const float v_ka = value_at(ka), v_kb = value_at(kb);
    if (time_at(ka) > a) integral_acc_piece(acc, method, time_at(ka - 1), value_at(ka - 1), time_at(ka), v_ka, a, time_at(ka));
    double integral = integral_acc_cell(acc).integral;
    if (kb > ka) {
        const double width = (double)delta;
        if (method == MDB_INTEGRAL_STEP) integral += width * sum_of(ka, kb - 1);
        else integral += width * (sum_of(ka, kb) - ((double)v_ka + (double)v_kb) * 0.5);
    }
    if (time_at(kb) < e) {
        acc = integral_acc_empty();
        integral_acc_piece(acc, method, time_at(kb), v_kb, time_at(kb + 1), value_at(kb + 1), time_at(kb), e);
        integral += integral_acc_cell(acc).integral;
    }
    cell.integral = integral;
    return cell;
}

// The host-side checks every form makes before it touches the device.
inline int integral_request_check(const mdb_integral_request *request, uint64_t *n_cells) {
    const mdb_bucket_request &b = request->buckets;
    if (b.which_mask != 0) return fail("which_mask must be 0 for mdb_integral_buckets*.");
    if (b.width <= 0) return fail("The bucket width must be positive.");
    if (b.n_groups == 0) return fail("n_groups must be at least 1.");
    if (b.t_lo != INT64_MIN || b.t_hi != INT64_MAX)
        return fail("mdb_integral_buckets* takes no time range: t_lo / t_hi must be INT64_MIN / INT64_MAX.");
    if (request->method != MDB_INTEGRAL_LINEAR && request->method != MDB_INTEGRAL_STEP)
        return fail("Unknown method: MDB_INTEGRAL_LINEAR or MDB_INTEGRAL_STEP.");
    if (request->flags != 0) return fail("mdb_integral_request.flags must be 0.");
    if (request->max_gap < 0) return fail("max_gap must not be negative.");
    const unsigned __int128 cells = (unsigned __int128)b.n_groups * b.n_buckets;
    if (cells * sizeof(mdb_integral_cell) > (unsigned __int128)UINT64_MAX) return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// mdb_integral.hip: the host batches of the list uploaded and folded into the caller's cells (the request checked,
// the list not empty). The only step of the host forms that needs the device.
int integral_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                      uint32_t n_inputs, const mdb_integral_request *request, uint64_t n_cells, mdb_integral_cell *inout);

} // namespace mdb

#if defined(__HIPCC__)

namespace mdb {

struct IntegralRequest { // what the kernels take: the buckets (no time range, which_mask 0), the gap rule, the method
    BucketRequest buckets;
    int64_t max_gap;
    uint32_t method;
};

struct IntegralHead { // the first row of a segment, as its left neighbour's link reads it (its time is start_time)
    float value;
    uint32_t rows; // 0: the segment rebuilds to no row
};

// mdb_integral.hip: k_integral_heads enqueued on the context's stream - heads[i] for every segment i > 0 whose left
// neighbour has pairs (offsets) and shares its group; the segments' errors are ORed into *error. Shared with
// mdb_sample.hip, whose links read the same heads.
void integral_heads_launch(mdb_ctx *ctx, const DevSegments &s, const uint32_t *groups, const unsigned long long *offsets,
                           IntegralHead *heads, unsigned int *error);

__device__ __forceinline__ bool integral_same_group(const uint32_t *groups, uint64_t i, uint64_t j) {
    return !groups || groups[i] == groups[j];
}

// The last instant segment i's function can reach: its right neighbour's first point when the two are linked by the
// segments' own times, else its end_time. (The rows decide in k_integral_partials; a last row before end_time only
// makes this extent larger than the function's.)
__device__ __forceinline__ int64_t integral_extent_end(const DevSegments &s, const uint32_t *groups, uint64_t i,
                                                       int64_t max_gap) {
    const int64_t end = s.end_time[i];
    if (i + 1 >= s.n || !integral_same_group(groups, i, i + 1)) return end;
    const int64_t next = s.start_time[i + 1];
    return integral_linked(max_gap, end, next) ? next : end;
}

__device__ __forceinline__ uint64_t integral_span(const DevSegments &s, const uint32_t *groups, uint64_t i,
                                                  const IntegralRequest &q, uint64_t *first) {
    return bucket_span(s.start_time[i], integral_extent_end(s, groups, i, q.max_gap), q.buckets, first);
}

// The head of segment i, whose analysis is `info` (no error in it): its rows and, when it has any, its first value.
// What k_integral_heads stores, shared with the heads kernel of mdb_transit.hip.
__device__ __forceinline__ IntegralHead integral_head_of(const DevSegments &s, uint64_t i, const SegInfo &info, uint32_t *error) {
    const SegDesc &d = info.desc;
    IntegralHead head = {0.0f, d.n_total};
    if (d.n_total == 0) return head;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    if (type == MDB_MACAQUE_V_ID) {
        const uint4 vv = s.values.views[i];
        decode_macaque_v(view_data(s.values, i, vv), vv.x, 1u, false, 0, error,
                         [&](uint32_t, uint32_t bits) { head.value = __uint_as_float(bits); });
    } else if (d.n_model > 0) {
        head.value = model_value_at(d, type, d.start);
    } else { // (a PMC-Mean segment whose every point is a residual)
        const uint4 vr = s.residuals.views[i];
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, 1u, true, __float_as_uint(d.value), error,
                         [&](uint32_t, uint32_t bits) { head.value = __uint_as_float(bits); });
    }
    return head;
}

// Every row of segment i in row order: emit(t, v). `limit` rows at most on regular timestamps (the caller knows
// how far its window reaches); irregular timestamps are decoded to the end. The walk of trend_stream_decode: the
// values decoded once, the timestamp beside each.
template <typename Emit>
__device__ __forceinline__ void integral_rows(const DevSegments &s, uint64_t i, const SegInfo &info, uint32_t limit,
                                              uint32_t *error, Emit emit) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const bool regular = (d.flags & FLAG_REGULAR) != 0;
    const uint32_t needed = regular ? min(limit, d.n_total) : d.n_total;
    const uint32_t n_res = d.n_total - d.n_model;
    if (needed == 0) return;
    TrendTimes times;
    if (!regular) times.open(s, i, d);
    auto time_of = [&](uint32_t k) { return regular ? trend_time_at(d, k) : times.next(k, error); };
    float seed = d.value;
    const bool residuals_needed = n_res > 0 && needed > d.n_model;
    if (type == MDB_MACAQUE_V_ID) {
        const uint4 vv = s.values.views[i];
        uint32_t last_bits = 0;
        decode_macaque_v(view_data(s.values, i, vv), vv.x, residuals_needed ? d.n_model : min(d.n_model, needed), false,
                         0, error, [&](uint32_t k, uint32_t bits) {
                             emit(time_of(k), __uint_as_float(bits));
                             last_bits = bits;
                         });
        seed = __uint_as_float(last_bits);
    } else if (d.n_model > 0) {
        const uint32_t upto = min(d.n_model, needed);
        if (regular) {
            for (uint32_t k = 0; k < upto; k++) {
                const int64_t t = trend_time_at(d, k);
                emit(t, model_value_at(d, type, t));
            }
        } else {
            times.first(upto, error, [&](uint32_t k, int64_t t) {
                if (k < d.n_model) emit(t, model_value_at(d, type, t));
            });
        }
    }
    if (residuals_needed) {
        const uint4 vr = s.residuals.views[i];
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, needed - d.n_model, true, __float_as_uint(seed), error,
                         [&](uint32_t k, uint32_t bits) { emit(time_of(d.n_model + k), __uint_as_float(bits)); });
    }
}

// Slots [j0, j1) of the slice (slot j: bucket b_first + (j - off)) for segment i, whose link to its right neighbour
// (same group; `head` its first row) is the segment's own. PMC-Mean and Swing on regular timestamps: each slot's
// share of the model in closed form, O(1); then only the residual tail and the link are walked, behind the model's
// last point. Everything else - MacaqueV values, irregular timestamps, a sampling interval the gap rule does not link
// - is one walk of the rows.
__device__ __forceinline__ void integral_segment_partials(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                          const IntegralRequest &q, uint64_t off, uint64_t b_first,
                                                          uint64_t j0, uint64_t j1, uint64_t p0,
                                                          mdb_integral_cell *__restrict__ out, bool neighbour,
                                                          const IntegralHead *__restrict__ heads, uint32_t *error) {
    const SegDesc &d = info.desc;
    const BucketRequest &r = q.buckets;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const bool regular = (d.flags & FLAG_REGULAR) != 0;
    IntegralWindow w = {r.origin, r.width, q.max_gap, b_first + (j0 - off), b_first + (j1 - off), q.method,
                        out + (j0 - p0)};
    // A model on regular timestamps: its rows need no walk, whether the gap rule links them (closed) or none of them.
    const bool model = regular && type != MDB_MACAQUE_V_ID && d.n_model >= 1;
    const bool closed = model && d.n_model >= 2 && integral_linked(q.max_gap, 0, d.delta);
    for (uint64_t j = j0; j < j1; j++) {
        mdb_integral_cell cell = {0, 0.0};
        if (closed) {
            const int64_t start = integral_bucket_start(r.origin, r.width, b_first + (j - off));
            cell = integral_regular_cell(
                q.method, d.start, d.delta, d.n_model, start, integral_bucket_end(start, r.width), type == MDB_PMC_MEAN_ID,
                [&](uint32_t k) { return model_value_at(d, type, trend_time_at(d, k)); },
                [&](uint32_t a, uint32_t b) {
                    RangeAcc acc;
                    model_closed_form(d, type, a, b, acc);
                    return acc.sum;
                });
        }
        out[j - p0] = cell;
    }
    // The link is walked when the rows' own rule may link it; the last row's time is arithmetic on regular timestamps
    // and end_time on irregular ones (the stream does not store it).
    const IntegralHead head = neighbour ? heads[i + 1] : IntegralHead{0.0f, 0u};
    const int64_t next = neighbour ? s.start_time[i + 1] : 0;
    const int64_t t_last = regular ? (d.n_total > 0 ? trend_time_at(d, d.n_total - 1) : d.start) : s.end_time[i];
    const bool link = neighbour && head.rows > 0 && d.n_total > 0 && integral_linked(q.max_gap, t_last, next);
    IntegralWalk walk = integral_walk_start();
    const uint32_t n_res = d.n_total - d.n_model;
    if (model) {
        if (n_res > 0 || link) integral_walk_point(w, walk, trend_time_at(d, d.n_model - 1), d.value);
        if (n_res > 0) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, n_res, true, __float_as_uint(d.value), error,
                             [&](uint32_t k, uint32_t bits) {
                                 integral_walk_point(w, walk, trend_time_at(d, d.n_model + k), __uint_as_float(bits));
                             });
        }
    } else {
        // How far the rows are needed on regular timestamps: to the end when the link wants the last value, else one
        // row past the window's last instant.
        uint32_t limit = d.n_total;
        if (regular && !link && d.delta > 0 && d.n_total > 0) {
            const int64_t window_end =
                integral_bucket_end(integral_bucket_start(r.origin, r.width, w.b1 - 1), r.width);
            if (window_end <= d.start) limit = 1;
            else if (window_end <= t_last) {
                const uint64_t to = (uint64_t)window_end - (uint64_t)d.start, step = (uint64_t)d.delta;
                limit = (uint32_t)min((uint64_t)d.n_total, to / step + (to % step != 0) + 1);
            }
        }
        integral_rows(s, i, info, limit, error, [&](int64_t t, float v) { integral_walk_point(w, walk, t, v); });
    }
    if (link) integral_walk_point(w, walk, next, head.value);
    integral_walk_flush(w, walk);
}

} // namespace mdb

#endif // __HIPCC__
