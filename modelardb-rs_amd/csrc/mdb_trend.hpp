// mdb_trend.hpp - the linear trend of a field over time (mdb_trend_buckets*): per date_bin bucket and group one
// mdb_comoments_cell with x = the time offset of a point inside its bucket and y = its value. regr_slope(field, ts),
// regr_r2, corr and covar_* follow from a cell with mdb_comoments_finish, unchanged.
//
// The first part is plain C++ (no HIP type): the x of a point, a run of points accumulated with shifted sums, the closed
// forms of the x side on regular timestamps and the checks of a request. It is shared by the kernels, by the host entry
// points (mdb_trend_host.cpp) and by the check program tests/trend_host, which runs it under the CPU sanitizers. The
// second part (hipcc only) is what one lane makes of one (segment, bucket) pair.
//
// A run is a ComomentsRun (mdb_comoments.hpp) summed around its first pair (x of the first point, its value). dx of a
// later point is the integer difference t - t_first converted to double - k * delta on regular timestamps - so no digit
// of a timestamp is lost at any epoch; dy = (double)v - (double)v_first. Runs meet only in comoments_merge.
//
// On regular timestamps the x side of n points at x0, x0 + delta, ... needs no point:
//   sum of dx = delta * n(n-1)/2      mean_x = x0 + delta * (n-1)/2      m2_x = delta^2 * n(n^2-1)/12
// n < 2^32, so n(n-1) < 2^64 is formed exactly in a uint64_t and converted once; every further factor is one f64
// operation, and the whole of m2_x carries at most seven roundings (below 2^-50 relative).
#pragma once

#include "mdb_comoments.hpp"

namespace mdb {

// The first instant of bucket b as a wrapped 64-bit value (bucket_bounds' arithmetic): t - trend_bucket_base(...) is the
// exact x of a timestamp t of that bucket, in [0, width).
MDB_MOMENTS_FN uint64_t trend_bucket_base(int64_t origin, int64_t width, uint64_t b) {
    return (uint64_t)origin + b * (uint64_t)width;
}

MDB_MOMENTS_FN double trend_x(int64_t t, uint64_t bucket_base) { return (double)((uint64_t)t - bucket_base); }

struct TrendRun {
    ComomentsRun sums;
    int64_t t_first;
};

MDB_MOMENTS_FN TrendRun trend_run_empty() { return TrendRun{comoments_run_empty(), 0}; }

// Point (t, v) of the bucket that starts at bucket_base. (t - t_first is below the width for the points of one bucket;
// it is taken signed, so a malformed stream whose timestamps go backwards still gives its true differences.)
MDB_MOMENTS_FN void trend_point(TrendRun &run, uint64_t bucket_base, int64_t t, float value) {
    ComomentsRun &c = run.sums;
    const double y = (double)value;
    if (c.n == 0) {
        run.t_first = t;
        c.kx = trend_x(t, bucket_base);
        c.ky = y;
    }
    const double dx = (double)(int64_t)((uint64_t)t - (uint64_t)run.t_first), dy = y - c.ky;
    c.sx += dx;
    c.sy += dy;
    c.sxx += dx * dx;
    c.syy += dy * dy;
    c.sxy += dx * dy;
    c.n++;
}

MDB_MOMENTS_FN mdb_comoments_cell trend_finish(const TrendRun &run) { return comoments_finish(run.sums); }

// n(n-1)/2 as a double: the sum of 0 .. n-1 (n < 2^32: the product is exact in 64 bits, one rounding).
MDB_MOMENTS_FN double trend_index_sum(uint64_t n) { return (double)(n * (n - 1) / 2); }

// The x side of n >= 1 points at x0 + k * delta, k in [0, n): the mean and m2 (see above). delta may be 0 (every
// point at one instant: m2_x is 0.0 exactly).
MDB_MOMENTS_FN void trend_regular_x(uint64_t n, double x0, double delta, double *mean_x, double *m2_x) {
    *mean_x = x0 + delta * ((double)(n - 1) * 0.5);
    // n(n^2-1)/12 = n(n-1) * (n+1) / 12
    *m2_x = delta * delta * ((double)(n * (n - 1)) * (double)(n + 1) / 12.0);
}

// The cell of n points of one value at x0 + k * delta (a PMC-Mean pair on regular timestamps), O(1). m2_y and c_xy:
// value - value, which is 0 - or NaN for a NaN or an infinity, as the sums over the points would be.
MDB_MOMENTS_FN mdb_comoments_cell trend_constant_cell(uint64_t n, double x0, double delta, float value) {
    mdb_comoments_cell cell = {0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n == 0) return cell;
    const double y = (double)value;
    cell.count = (int64_t)n;
    trend_regular_x(n, x0, delta, &cell.mean_x, &cell.m2_x);
    cell.mean_y = y;
    cell.m2_y = y - y;
    cell.c_xy = y - y;
    return cell;
}

// The cell of n points at x0 + k * delta whose y side was summed around the first value ky with dx = k * delta:
// sy, syy and sxy as in a ComomentsRun (a Swing pair on regular timestamps). The x side is the closed form; c_xy uses
// the sum of dx = delta * n(n-1)/2.
MDB_MOMENTS_FN mdb_comoments_cell trend_regular_cell(uint64_t n, double x0, double delta, double ky, double sy, double syy,
                                                     double sxy) {
    mdb_comoments_cell cell = {0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n == 0) return cell;
    const double count = (double)n;
    const double sx = delta * trend_index_sum(n);
    double m2_y = syy - sy * sy / count;
    if (m2_y < 0.0) m2_y = 0.0;
    cell.count = (int64_t)n;
    trend_regular_x(n, x0, delta, &cell.mean_x, &cell.m2_x);
    cell.mean_y = ky + sy / count;
    cell.m2_y = m2_y;
    cell.c_xy = sxy - sx * sy / count;
    return cell;
}

// The host-side checks every form makes before it touches the device: those of mdb_moments_buckets*.
inline int trend_request_check(const mdb_bucket_request *request, uint64_t *n_cells) {
    if (request->which_mask != 0) return fail("which_mask must be 0 for mdb_trend_buckets*.");
    if (request->width <= 0) return fail("The bucket width must be positive.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    const unsigned __int128 cells = (unsigned __int128)request->n_groups * request->n_buckets;
    if (cells * sizeof(mdb_comoments_cell) > (unsigned __int128)UINT64_MAX) return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// mdb_trend.hip: the host batches of the list uploaded and folded into the caller's cells (the request checked, the
// list not empty). The only step of the host forms that needs the device.
int trend_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                   uint32_t n_inputs, const mdb_bucket_request *request, uint64_t n_cells, mdb_comoments_cell *inout);

} // namespace mdb

#if defined(__HIPCC__)

namespace mdb {

__device__ __forceinline__ int64_t trend_time_at(const SegDesc &d, uint32_t k) {
    return d.start + (int64_t)((uint64_t)k * (uint64_t)d.delta);
}

// The model points [a, b] of a PMC-Mean or Swing segment with regular timestamps inside the bucket that starts at
// bucket_base, merged into `acc`. PMC-Mean: O(1), no loop. Swing: the x side in closed form, the y side point by point
// in registers - the rebuilt points are f32 roundings of the line (moments_model_points, mdb_moments.hpp, says why
// that has no closed form).
__device__ __forceinline__ void trend_model_points(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b,
                                                   uint64_t bucket_base, mdb_comoments_cell &acc) {
    const uint64_t n = (uint64_t)(b - a) + 1;
    int64_t t = trend_time_at(d, a);
    const double x0 = trend_x(t, bucket_base), delta = (double)d.delta;
    if (type == MDB_PMC_MEAN_ID) {
        comoments_merge(acc, trend_constant_cell(n, x0, delta, d.value));
        return;
    }
    const double ky = (double)(float)(d.slope * (double)t + d.intercept);
    double sy = 0.0, syy = 0.0, sxy = 0.0;
    uint64_t step = 0; // (index - a) * delta = t - t_first, wrapping-exact
    for (uint32_t index = a;; index++) {
        const double dy = (double)(float)(d.slope * (double)t + d.intercept) - ky;
        const double dx = (double)(int64_t)step;
        sy += dy;
        syy += dy * dy;
        sxy += dx * dy;
        if (index == b) break;
        t = (int64_t)((uint64_t)t + (uint64_t)d.delta);
        step += (uint64_t)d.delta;
    }
    comoments_merge(acc, trend_regular_cell(n, x0, delta, ky, sy, syy, sxy));
}

// The points of a PMC-Mean or Swing segment with regular timestamps inside [lo, hi] of the bucket that starts at
// bucket_base: the model's as above, the residual tail's decoded as a run of its own (not when the tail is
// k_trend_pieces').
__device__ __forceinline__ mdb_comoments_cell trend_regular_pair(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                                 int64_t lo, int64_t hi, uint64_t bucket_base,
                                                                 uint32_t *error, bool tail_by_pieces) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const uint32_t n_res = d.n_total - d.n_model;
    mdb_comoments_cell acc = comoments_empty();
    uint32_t k_lo = 0, k_hi = 0;
    if (!regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi)) return acc;
    if (k_lo < d.n_model) trend_model_points(d, type, k_lo, min(k_hi, d.n_model - 1), bucket_base, acc);
    if (n_res > 0 && k_hi >= d.n_model && !tail_by_pieces) {
        const uint4 vr = s.residuals.views[i];
        TrendRun run = trend_run_empty();
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, k_hi - d.n_model + 1, true, __float_as_uint(d.value),
                         error, [&](uint32_t k, uint32_t bits) {
                             const uint32_t index = d.n_model + k;
                             if (index >= k_lo) trend_point(run, bucket_base, trend_time_at(d, index), __uint_as_float(bits));
                         });
        comoments_merge(acc, trend_finish(run));
    }
    return acc;
}

// The timestamps of an irregular segment one after the other, for a walk whose outer loop is the value decoder: next(k)
// must be asked for k = 0, 1, 2, ... in order. Each call resumes decode_irregular_span where the last one stopped.
struct TrendTimes {
    const uint8_t *bytes;
    uint32_t nbytes;
    int64_t start, end;
    TsCursor at;
    __device__ __forceinline__ void open(const DevSegments &s, uint64_t i, const SegDesc &d) {
        const uint4 vt = s.timestamps.views[i];
        bytes = view_data(s.timestamps, i, vt);
        nbytes = vt.x;
        start = d.start;
        end = s.end_time[i];
        at = ts_stream_start(d.start);
    }
    // Points [0, limit) in one go, before any next(): emit(k, t) for each; next(limit) may follow.
    template <typename Emit>
    __device__ __forceinline__ void first(uint32_t limit, uint32_t *error, Emit emit) {
        if (limit == 0) return;
        emit(0u, start);
        if (limit == 1) return;
        bool finished;
        at = decode_irregular_span(bytes, nbytes, end, limit, error, at, 0xffffffffu, &finished, emit,
                                   [](const TsCursor &) {});
    }
    __device__ __forceinline__ int64_t next(uint32_t k, uint32_t *error) {
        if (k == 0) return start;
        int64_t t = at.timestamp;
        bool finished;
        at = decode_irregular_span(bytes, nbytes, end, k + 1, error, at, 0xffffffffu, &finished,
                                   [&](uint32_t, int64_t time) { t = time; }, [](const TsCursor &) {});
        return t;
    }
};

// Pass 2 over the slots [j0, j1) of a segment whose points are a bit stream, each slot holding its index interval
// (ascending, disjoint; slot j is bucket b_first + (j - off)): the values are decoded once, up to point `needed` - 1,
// each with its timestamp into the run of the slot whose interval holds it, and every slot is overwritten with the
// cell of its run (m4_stream_decode's walk: the timestamp travels beside the value). Regular timestamps are
// arithmetic; irregular ones come from the timestamp stream in step with the values (TrendTimes).
__device__ __forceinline__ void trend_stream_decode(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                    const BucketRequest &r, uint64_t off, uint64_t b_first, uint64_t j0,
                                                    uint64_t j1, uint64_t p0, mdb_comoments_cell *__restrict__ out,
                                                    uint32_t needed, uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const uint32_t n_res = d.n_total - d.n_model;
    const bool regular = (d.flags & FLAG_REGULAR) != 0;
    uint64_t j = j0;
    uint2 current = comoments_interval(&out[j - p0]);
    uint64_t base = trend_bucket_base(r.origin, r.width, b_first + (j - off));
    TrendRun run = trend_run_empty();
    auto flush = [&]() {
        out[j - p0] = trend_finish(run);
        run = trend_run_empty();
        j++;
        base += (uint64_t)r.width;
        if (j < j1) current = comoments_interval(&out[j - p0]);
    };
    auto visit = [&](uint32_t k, int64_t t, float v) {
        while (j < j1 && k > current.y) flush();
        if (j < j1 && k >= current.x) trend_point(run, base, t, v);
    };
    if (needed > 0) {
        TrendTimes times;
        if (!regular) times.open(s, i, d);
        auto time_of = [&](uint32_t k) { return regular ? trend_time_at(d, k) : times.next(k, error); };
        float seed = d.value;
        if (type == MDB_MACAQUE_V_ID) {
            const uint4 vv = s.values.views[i];
            uint32_t last_bits = 0;
            const bool residuals_needed = n_res > 0 && needed > d.n_model;
            decode_macaque_v(view_data(s.values, i, vv), vv.x, residuals_needed ? d.n_model : min(d.n_model, needed),
                             false, 0, error, [&](uint32_t k, uint32_t bits) {
                                 visit(k, time_of(k), __uint_as_float(bits));
                                 last_bits = bits;
                             });
            seed = __uint_as_float(last_bits);
        } else if (d.n_model > 0) { // PMC-Mean / Swing on irregular timestamps: the model at each timestamp
            times.first(min(d.n_model, needed), error, [&](uint32_t k, int64_t t) {
                if (k < d.n_model) visit(k, t, model_value_at(d, type, t));
            });
        }
        if (n_res > 0 && needed > d.n_model) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, needed - d.n_model, true, __float_as_uint(seed),
                             error, [&](uint32_t k, uint32_t bits) {
                                 visit(d.n_model + k, time_of(d.n_model + k), __uint_as_float(bits));
                             });
        }
    }
    while (j < j1) flush();
}

// The pairs of a segment whose points are a bit stream (MacaqueV values, irregular timestamps): slots [j0, j1) of the
// slice, buckets b_first + (j - off), as moments_stream_partials - pass 1 leaves each slot's index interval,
// trend_stream_decode does the rest. Returns false when the timestamps turn out not to be sorted (a malformed stream):
// the caller then goes pair by pair (trend_unsorted_pair).
__device__ __forceinline__ bool trend_stream_partials(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                      const BucketRequest &r, uint64_t off, uint64_t b_first, uint64_t j0,
                                                      uint64_t j1, uint64_t p0, mdb_comoments_cell *__restrict__ out,
                                                      uint32_t *error) {
    const SegDesc &d = info.desc;
    const int64_t end = s.end_time[i];
    uint32_t needed = 0; // points [0, needed) reach a slot
    if (d.flags & FLAG_REGULAR) {
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
        bool sorted = true;
        decode_irregular_timestamps(view_data(s.timestamps, i, vt), vt.x, d.start, end, 0xffffffffu, error,
                                    [&](uint32_t k, int64_t t) {
                                        if (t < previous) sorted = false;
                                        previous = t;
                                        if (!sorted || t < r.t_lo || t > r.t_hi || t < r.origin) return;
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
    trend_stream_decode(s, i, info, r, off, b_first, j0, j1, p0, out, needed, error);
    return true;
}

// One pair [lo, hi] (slot j, bucket b_first + (j - off)) of a segment with irregular timestamps that are not sorted (a
// malformed stream): the points the range aggregate counts for the same bounds (segment_range, mdb_agg_dev.hpp), as
// moments_unsorted_pair. A model without residuals: every point is tested with its own timestamp. Values in a bit
// stream: the indices between the first and the last timestamp inside [lo, hi], each with its own timestamp.
__device__ __forceinline__ void trend_unsorted_pair(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                    const BucketRequest &r, uint64_t off, uint64_t b_first, int64_t lo,
                                                    int64_t hi, uint64_t j, uint64_t p0,
                                                    mdb_comoments_cell *__restrict__ out, uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint4 vt = s.timestamps.views[i];
    const uint8_t *ts_bytes = view_data(s.timestamps, i, vt);
    if (type != MDB_MACAQUE_V_ID && d.n_total == d.n_model) {
        const uint64_t base = trend_bucket_base(r.origin, r.width, b_first + (j - off));
        TrendRun run = trend_run_empty();
        if (!(end < lo || d.start > hi))
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t, int64_t t) {
                if (t >= lo && t <= hi) trend_point(run, base, t, model_value_at(d, type, t));
            });
        out[j - p0] = trend_finish(run);
        return;
    }
    uint32_t k_lo = 0xffffffffu, k_hi = 0;
    if (!(end < lo || d.start > hi))
        decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t k, int64_t t) {
            if (t >= lo && t <= hi) {
                if (k < k_lo) k_lo = k;
                if (k > k_hi) k_hi = k;
            }
        });
    const bool any = k_lo != 0xffffffffu;
    comoments_set_interval(&out[j - p0], any ? k_lo : 1u, any ? k_hi : 0u);
    trend_stream_decode(s, i, info, r, off, b_first, j, j + 1, p0, out, any ? k_hi + 1 : 0, error);
}

} // namespace mdb

#endif // __HIPCC__
