// mdb_moments.hpp - variance and standard deviation (mdb_moments_buckets*): the count, the mean and m2 = the sum of
// (v - mean)^2 of every date_bin bucket and group.
//
// The first part is plain C++ (no HIP type): a run of points accumulated with shifted sums, the merge rule on cells,
// and the checks of a request. It is shared by the kernels, by the host entry points (mdb_moments_host.cpp) and by the
// check program tests/moments_host, which runs it under the CPU sanitizers. The second part (hipcc only) is what one
// lane makes of one (segment, bucket) pair.
//
// A run - the points of one pair, or of one piece inside one bucket - is summed around its first value K:
//   d = (double)v - (double)K     s1 += d     s2 += d * d     at the end: mean = K + s1 / n, m2 = s2 - s1 * s1 / n
// Two f64 operations a point and no division (a Welford update has one per point). K is one of the run's points, so
// s1 * s1 / n is at most n times m2: what cancels in the last step is bounded by the run's length, not by the level
// of the values as with a sum of v * v. Runs are combined by the merge rule only (moments_merge).
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include "mdb_bucket_fold.hpp"
#define MDB_MOMENTS_FN __host__ __device__ __forceinline__
#else
#include "mdb_host_side.hpp"
#define MDB_MOMENTS_FN inline
#endif

namespace mdb {

struct MomentsRun {
    int64_t n;
    double k, s1, s2;
};

MDB_MOMENTS_FN MomentsRun moments_run_empty() { return MomentsRun{0, 0.0, 0.0, 0.0}; }

MDB_MOMENTS_FN void moments_point(MomentsRun &run, float v) {
    const double x = (double)v;
    run.k = run.n == 0 ? x : run.k;
    const double d = x - run.k;
    run.s1 += d;
    run.s2 += d * d;
    run.n++;
}

// The cell of a run; an empty run gives a fresh cell. m2 is clamped at 0 when it rounds below (a comparison, not
// fmax: a NaN stays one).
MDB_MOMENTS_FN mdb_moments_cell moments_finish(const MomentsRun &run) {
    mdb_moments_cell cell = {0, 0.0, 0.0};
    if (run.n == 0) return cell;
    const double n = (double)run.n;
    double m2 = run.s2 - run.s1 * run.s1 / n;
    if (m2 < 0.0) m2 = 0.0;
    cell.count = run.n;
    cell.mean = run.k + run.s1 / n;
    cell.m2 = m2;
    return cell;
}

// The points of `from` added to those of `into`. An empty `from` changes nothing; an empty `into` (count 0: no other
// member is read) takes every member of `from`. Equal means: d = 0, so mean and a zero m2 stay what they are, exactly.
MDB_MOMENTS_FN void moments_merge(mdb_moments_cell &into, const mdb_moments_cell &from) {
    if (from.count == 0) return;
    if (into.count == 0) {
        into = from;
        return;
    }
    const double na = (double)into.count, nb = (double)from.count;
    const int64_t count = into.count + from.count;
    const double n = (double)count;
    const double d = from.mean - into.mean;
    into.mean = into.mean + d * (nb / n);
    into.m2 = into.m2 + from.m2 + d * d * (na * nb / n);
    into.count = count;
}

// The host-side checks every form makes before it touches the device: those of mdb_m4_buckets*.
inline int moments_request_check(const mdb_bucket_request *request, uint64_t *n_cells) {
    if (request->which_mask != 0) return fail("which_mask must be 0 for mdb_moments_buckets*.");
    if (request->width <= 0) return fail("The bucket width must be positive.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    const unsigned __int128 cells = (unsigned __int128)request->n_groups * request->n_buckets;
    if (cells * sizeof(mdb_moments_cell) > (unsigned __int128)UINT64_MAX) return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// mdb_moments.hip: the host batches of the list uploaded and folded into the caller's cells (the request checked, the
// list not empty). The only step of the host forms that needs the device.
int moments_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                     uint32_t n_inputs, const mdb_bucket_request *request, uint64_t n_cells, mdb_moments_cell *inout);

} // namespace mdb

#if defined(__HIPCC__)

namespace mdb {

__device__ __forceinline__ mdb_moments_cell moments_empty() { return mdb_moments_cell{0, 0.0, 0.0}; }

// What the tree and fold (mdb_bucket_fold.hpp) need to know of a moments cell: for mdb_moments.hip and for
// mdb_binned.hip, whose partials are moments cells too (each instantiates BucketFold<MomentsFoldOps> itself).
struct MomentsFoldOps : FoldOps<mdb_moments_cell> {
    static constexpr const char *tree_name = "k_moments_tree", *fold_name = "k_moments_fold";
    __device__ __forceinline__ static mdb_moments_cell empty() { return moments_empty(); }
    __device__ __forceinline__ static void merge(mdb_moments_cell &into, const mdb_moments_cell &from) { moments_merge(into, from); }
    __device__ __forceinline__ static bool is_empty(const mdb_moments_cell &acc) { return acc.count == 0; }
    __device__ __forceinline__ void apply(mdb_moments_cell &cell, const mdb_moments_cell &acc) const { moments_merge(cell, acc); }
};

// The model points [a, b] of a PMC-Mean or Swing segment with regular timestamps, merged into `acc`. PMC-Mean: n equal
// values, exact in O(1). Swing: (float)(slope * t + intercept) point by point in registers - the rebuilt points are f32
// roundings of the line, and for a line that rises little against its level that rounding is the larger part of the
// variance, so the variance of the unrounded line (a closed form) is a different number.
__device__ __forceinline__ void moments_model_points(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b,
                                                     mdb_moments_cell &acc) {
    const int64_t n = (int64_t)(b - a) + 1;
    if (type == MDB_PMC_MEAN_ID) {
        const double value = (double)d.value;
        moments_merge(acc, mdb_moments_cell{n, value, value - value}); // (m2: 0, or NaN for a NaN or an infinity)
        return;
    }
    int64_t t = d.start + (int64_t)((uint64_t)a * (uint64_t)d.delta);
    const double k = (double)(float)(d.slope * (double)t + d.intercept);
    double s1 = 0.0, s2 = 0.0; // (point a itself: d = k - k, which is 0 - or NaN for a non-finite k, as it must be)
    for (uint32_t index = a;; index++) {
        const double x = (double)(float)(d.slope * (double)t + d.intercept) - k;
        s1 += x;
        s2 += x * x;
        if (index == b) break;
        t = (int64_t)((uint64_t)t + (uint64_t)d.delta);
    }
    moments_merge(acc, moments_finish(MomentsRun{n, k, s1, s2}));
}

// The points of a PMC-Mean or Swing segment with regular timestamps inside [lo, hi]: the model's as above, the
// residual tail's decoded as a run of its own (not when the tail is k_moments_pieces').
__device__ __forceinline__ mdb_moments_cell moments_regular_pair(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                                 int64_t lo, int64_t hi, uint32_t *error,
                                                                 bool tail_by_pieces) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const uint32_t n_res = d.n_total - d.n_model;
    mdb_moments_cell acc = moments_empty();
    uint32_t k_lo = 0, k_hi = 0;
    if (!regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi)) return acc;
    if (k_lo < d.n_model) moments_model_points(d, type, k_lo, min(k_hi, d.n_model - 1), acc);
    if (n_res > 0 && k_hi >= d.n_model && !tail_by_pieces) {
        const uint4 vr = s.residuals.views[i];
        MomentsRun run = moments_run_empty();
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, k_hi - d.n_model + 1, true, __float_as_uint(d.value),
                         error, [&](uint32_t k, uint32_t bits) {
                             if (d.n_model + k >= k_lo) moments_point(run, __uint_as_float(bits));
                         });
        moments_merge(acc, moments_finish(run));
    }
    return acc;
}

// Where pass 1 of a stream leaves slot j's index interval [x, y] of points (x > y: none): the cell's first 8 bytes.
// (Copied as bytes: the slot is read and written as a cell too.)
__device__ __forceinline__ uint2 moments_interval(const mdb_moments_cell *slot) {
    uint2 interval;
    __builtin_memcpy(&interval, slot, 8);
    return interval;
}
__device__ __forceinline__ void moments_set_interval(mdb_moments_cell *slot, uint32_t k_lo, uint32_t k_hi) {
    const uint2 interval = make_uint2(k_lo, k_hi);
    __builtin_memcpy(slot, &interval, 8);
}

// Pass 2 over the slots [j0, j1) of a segment whose points are a bit stream, each slot holding its index interval
// (ascending, disjoint): the values are decoded once, up to point `needed` - 1, each into the run of the slot whose
// interval holds it, and every slot is overwritten with the cell of its run (m4_stream_decode without the timestamps).
__device__ __forceinline__ void moments_stream_decode(const DevSegments &s, uint64_t i, const SegInfo &info, uint64_t j0,
                                                      uint64_t j1, uint64_t p0, mdb_moments_cell *__restrict__ out,
                                                      uint32_t needed, uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint32_t n_res = d.n_total - d.n_model;
    uint64_t j = j0;
    uint2 current = moments_interval(&out[j - p0]);
    MomentsRun run = moments_run_empty();
    auto flush = [&]() {
        out[j - p0] = moments_finish(run);
        run = moments_run_empty();
        j++;
        if (j < j1) current = moments_interval(&out[j - p0]);
    };
    auto visit = [&](uint32_t k, float v) {
        while (j < j1 && k > current.y) flush();
        if (j < j1 && k >= current.x) moments_point(run, v);
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
// slice, buckets b_first + (j - off), as m4_stream_partials (mdb_m4.hpp) - pass 1 leaves each slot's index interval,
// moments_stream_decode does the rest. Returns false when the timestamps turn out not to be sorted (a malformed
// stream): the caller then goes pair by pair (moments_unsorted_pair).
__device__ __forceinline__ bool moments_stream_partials(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                        const BucketRequest &r, uint64_t off, uint64_t b_first,
                                                        uint64_t j0, uint64_t j1, uint64_t p0,
                                                        mdb_moments_cell *__restrict__ out, uint32_t *error) {
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
            moments_set_interval(&out[j - p0], k_lo, k_hi);
        }
    } else {
        for (uint64_t j = j0; j < j1; j++) moments_set_interval(&out[j - p0], 1, 0);
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
                                            if (slot != ~0ull) moments_set_interval(&out[slot - p0], k_lo, k_hi);
                                            slot = j;
                                            k_lo = k;
                                        }
                                        k_hi = k;
                                    });
        if (!sorted) return false;
        if (slot != ~0ull) {
            moments_set_interval(&out[slot - p0], k_lo, k_hi);
            needed = k_hi + 1;
        }
    }
    moments_stream_decode(s, i, info, j0, j1, p0, out, needed, error);
    return true;
}

// One pair [lo, hi] of a segment with irregular timestamps that are not sorted (a malformed stream), into *slot: the
// points the range aggregate counts for the same bounds (segment_range, mdb_agg_dev.hpp), as m4_unsorted_pair. A model
// without residuals: every point is tested with its own timestamp. Values in a bit stream: the indices between the
// first and the last timestamp inside [lo, hi].
__device__ __forceinline__ void moments_unsorted_pair(const DevSegments &s, uint64_t i, const SegInfo &info, int64_t lo,
                                                      int64_t hi, uint64_t j, uint64_t p0,
                                                      mdb_moments_cell *__restrict__ out, uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint4 vt = s.timestamps.views[i];
    const uint8_t *ts_bytes = view_data(s.timestamps, i, vt);
    if (type != MDB_MACAQUE_V_ID && d.n_total == d.n_model) {
        MomentsRun run = moments_run_empty();
        if (!(end < lo || d.start > hi))
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t, int64_t t) {
                if (t >= lo && t <= hi) moments_point(run, model_value_at(d, type, t));
            });
        out[j - p0] = moments_finish(run);
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
    moments_set_interval(&out[j - p0], any ? k_lo : 1u, any ? k_hi : 0u);
    moments_stream_decode(s, i, info, j, j + 1, p0, out, any ? k_hi + 1 : 0, error);
}

} // namespace mdb

#endif // __HIPCC__
