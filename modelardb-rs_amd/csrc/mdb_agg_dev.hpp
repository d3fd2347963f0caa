// mdb_agg_dev.hpp - the points of one segment inside a time range, aggregated without materialising them
// (segment_range: ONE walk of a segment's model and streams, with a selector that says which points count - every one,
// by value, or by row): shared by the time-range, filtered and masked aggregates (mdb_agg.hip: k_agg_range,
// k_agg_filter, k_agg_mask) and the bucketed ones (mdb_buckets.hip).
#pragma once

#include "mdb_filter.hpp"
#include "mdb_segment_dev.hpp"

#include <cfloat>

namespace mdb {

struct RangeAcc {
    double sum = 0.0;
    long long count = 0;
    float min = FLT_MAX;
    float max = -FLT_MAX;
    __device__ __forceinline__ void point(float v) {
        sum += (double)v;
        count += 1;
        min = min_num(min, v);
        max = max_num(max, v);
    }
    __device__ __forceinline__ void merge(const RangeAcc &other) {
        sum += other.sum;
        count += other.count;
        min = min_num(min, other.min);
        max = max_num(max, other.max);
    }
};
static_assert(sizeof(RangeAcc) == 24, "arrays of partials are laid out in scratch by this size");

__device__ __forceinline__ float model_value_at(const SegDesc &d, uint32_t type, int64_t t) {
    return type == MDB_PMC_MEAN_ID ? d.value : (float)(d.slope * (double)t + d.intercept);
}

// The model points [a, b] of a PMC-Mean or Swing segment with regular timestamps, in closed form.
__device__ __forceinline__ void model_closed_form(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b,
                                                  RangeAcc &acc) {
    const uint32_t n = b - a + 1;
    const int64_t ta = d.start + (int64_t)((uint64_t)a * (uint64_t)d.delta);
    const int64_t tb = d.start + (int64_t)((uint64_t)b * (uint64_t)d.delta);
    const float va = model_value_at(d, type, ta);
    const float vb = model_value_at(d, type, tb);
    // (float)(slope * t + intercept) is monotone in t, so the extremes sit at the ends.
    acc.min = min_num(acc.min, min_num(va, vb));
    acc.max = max_num(acc.max, max_num(va, vb));
    acc.count += n;
    if (type == MDB_PMC_MEAN_ID) {
        acc.sum += (double)d.value * (double)n;
    } else {
        // Sum of the line over n equally spaced points: the f64 closed form of the f32 values
        // grid() would produce - unless it could miss their sum by more than a tenth of the
        // 0.001 % the reference allows (integration_test.rs:1155-1171). That happens when
        // slope * t + intercept cancels almost completely (epoch timestamps, a model that lasts
        // microseconds, values near zero): every reconstructed point then carries rounding noise
        // of ulp(slope * t), which averages out over the points but not over the two end points
        // the closed form uses. The bound below is the worst case of that noise plus the f32
        // rounding of the points; beyond it the points are summed one by one, which is exactly
        // what the reference's plan (GridExec + filter + SUM) computes.
        const double fa = d.slope * (double)ta + d.intercept;
        const double fb = d.slope * (double)tb + d.intercept;
        const double closed = (fa + fb) / 2.0 * (double)n;
        const double magnitude = fmax(fabs(fa), fabs(fb));
        const double cancelled = fmax(fmax(fabs(d.slope * (double)ta), fabs(d.slope * (double)tb)),
                                      fabs(d.intercept));
        const double worst = (double)n * (6.0e-8 * magnitude + 7.0e-46 + 2.3e-16 * cancelled);
        if (worst <= 1.0e-6 * fabs(closed)) {
            acc.sum += closed;
        } else {
            double pointwise = 0.0;
            for (uint32_t k = a; k <= b; k++) {
                const int64_t t = d.start + (int64_t)((uint64_t)k * (uint64_t)d.delta);
                pointwise += (double)model_value_at(d, type, t);
            }
            acc.sum += pointwise;
        }
    }
}

// What the two selectors of mdb_filter.hpp make of the model points [a, b]: all of them in closed form, or ...
__device__ __forceinline__ void AllValues::model(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, uint64_t,
                                                 RangeAcc &acc) const {
    model_closed_form(d, type, a, b, acc);
}
// ... the passing ones: none, one interval in closed form, or (an end is NaN) one by one.
__device__ __forceinline__ void ValueKeys::model(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, uint64_t,
                                                 RangeAcc &acc) const {
    uint32_t ra = a, rb = b;
    const int run = model_run(d, type, a, b, *this, &ra, &rb);
    if (run == RUN_INTERVAL) {
        model_closed_form(d, type, ra, rb, acc);
    } else if (run == RUN_POINTS) {
        for (uint32_t k = a; k <= b; k++) {
            const float v = model_value_at(d, type, d.start + (int64_t)((uint64_t)k * (uint64_t)d.delta));
            if (pass(v)) acc.point(v);
        }
    }
}

// Aggregate the points of segment i whose timestamp lies in [t_lo, t_hi] and which `sel` selects (mdb_filter.hpp:
// every one for the range calls, by value for the filtered ones; mdb_mask.hpp: by row for the masked ones). The row
// of a point is its position among the segment's points inside the range.
// tail_by_pieces: the residual tail's points are k_agg_mv_range's (regular timestamps only; never with rows).
template <typename Sel = AllValues>
__device__ __forceinline__ void segment_range(const DevSegments &s, uint64_t i, const SegInfo &info,
                                              int64_t t_lo, int64_t t_hi, RangeAcc &acc,
                                              uint32_t *error, bool tail_by_pieces = false,
                                              const Sel &sel = Sel()) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint32_t n_res = d.n_total - d.n_model;
    if (!(d.flags & FLAG_REGULAR)) {
        // Irregular timestamps: one serial pass, every point tested.
        if (end < t_lo || d.start > t_hi) return;
        const uint4 vt = s.timestamps.views[i];
        const uint8_t *ts_bytes = view_data(s.timestamps, i, vt);
        if (type != MDB_MACAQUE_V_ID && n_res == 0) {
            uint64_t row = 0; // (a running count, not k - k_lo: the two differ for a malformed, unsorted stream)
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error,
                                        [&](uint32_t, int64_t t) {
                                            if (t >= t_lo && t <= t_hi) {
                                                const float v = model_value_at(d, type, t);
                                                if (sel.counts(v, row)) acc.point(v);
                                                row += 1;
                                            }
                                        });
            return;
        }
        // Values are a bitstream too (MacaqueV model or residual tail): first find the index
        // interval of the in-range timestamps, then decode the values once. Rare combination.
        uint32_t k_lo = 0xffffffffu, k_hi = 0;
        decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error,
                                    [&](uint32_t k, int64_t t) {
                                        if (t >= t_lo && t <= t_hi) {
                                            if (k < k_lo) k_lo = k;
                                            if (k > k_hi) k_hi = k;
                                        }
                                    });
        if (k_lo == 0xffffffffu) return;
        // Timestamps are sorted, so the in-range points are exactly the indices k_lo..k_hi; point k is row k - k_lo.
        float seed = d.value;
        if (type == MDB_MACAQUE_V_ID) {
            const uint4 vv = s.values.views[i];
            uint32_t last_bits = 0;
            decode_macaque_v(view_data(s.values, i, vv), vv.x, d.n_model, false, 0, error,
                             [&](uint32_t k, uint32_t bits) {
                                 if (k >= k_lo && k <= k_hi) { if (sel.counts(__uint_as_float(bits), k - k_lo)) acc.point(__uint_as_float(bits)); }
                                 last_bits = bits;
                             });
            seed = __uint_as_float(last_bits);
        } else {
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, d.n_model, error,
                                        [&](uint32_t k, int64_t t) {
                                            if (k >= k_lo && k <= k_hi)
                                                { const float v = model_value_at(d, type, t); if (sel.counts(v, k - k_lo)) acc.point(v); }
                                        });
        }
        if (n_res > 0) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, n_res, true,
                             __float_as_uint(seed), error, [&](uint32_t k, uint32_t bits) {
                                 uint32_t index = d.n_model + k;
                                 if (index >= k_lo && index <= k_hi) { if (sel.counts(__uint_as_float(bits), index - k_lo)) acc.point(__uint_as_float(bits)); }
                             });
        }
        return;
    }

    // Regular timestamps start + k * delta: the in-range indices are an interval [k_lo, k_hi]; point k is row k - k_lo.
    uint32_t k_lo = 0, k_hi = 0;
    if (!regular_index_interval(d.start, d.delta, d.n_total, t_lo, t_hi, &k_lo, &k_hi)) return;

    // Model part [a, b] of the interval.
    if (type != MDB_MACAQUE_V_ID && k_lo < d.n_model) sel.model(d, type, k_lo, min(k_hi, d.n_model - 1), 0, acc);
    float seed = d.value;
    if (type == MDB_MACAQUE_V_ID) {
        const uint4 vv = s.values.views[i];
        uint32_t last_bits = 0;
        // Decode only as far as needed unless the residual seed (last value) is needed too.
        const bool residuals_in_range = n_res > 0 && k_hi >= d.n_model;
        const uint32_t upto = residuals_in_range ? d.n_model : min(d.n_model, k_hi + 1);
        if (k_lo < d.n_model || residuals_in_range) {
            decode_macaque_v(view_data(s.values, i, vv), vv.x, upto, false, 0, error,
                             [&](uint32_t k, uint32_t bits) {
                                 if (k >= k_lo && k <= k_hi) { if (sel.counts(__uint_as_float(bits), k - k_lo)) acc.point(__uint_as_float(bits)); }
                                 last_bits = bits;
                             });
        }
        seed = __uint_as_float(last_bits);
    }
    if (n_res > 0 && k_hi >= d.n_model && !tail_by_pieces) {
        const uint4 vr = s.residuals.views[i];
        const uint32_t upto = k_hi - d.n_model + 1;
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, upto, true, __float_as_uint(seed),
                         error, [&](uint32_t k, uint32_t bits) {
                             uint32_t index = d.n_model + k;
                             if (index >= k_lo) { if (sel.counts(__uint_as_float(bits), index - k_lo)) acc.point(__uint_as_float(bits)); }
                         });
    }
}

// ---- date_bin buckets (mdb_buckets.hip) ---------------------------------------------------------------------

struct BucketPartial { // one pair's points, or a run's: the layout of mdb_agg_state
    double sum;
    long long count;
    float min;
    float max;
};
static_assert(sizeof(BucketPartial) == sizeof(mdb_agg_state), "partials are cells");

struct BucketRequest {
    int64_t origin;
    int64_t width;
    uint64_t n_buckets;
    int64_t t_lo;
    int64_t t_hi;
    uint32_t n_groups;
    uint32_t which_mask;
};

__host__ __device__ __forceinline__ BucketPartial bucket_empty() { return BucketPartial{0.0, 0, FLT_MAX, -FLT_MAX}; }

__device__ __forceinline__ void bucket_add(BucketPartial &into, const BucketPartial &from) {
    into.sum += from.sum;
    into.count += from.count;
    into.min = min_num(into.min, from.min);
    into.max = max_num(into.max, from.max);
}

// The buckets segment [start, end] reaches once clipped by [t_lo, t_hi] and buckets 0 .. n_buckets-1: [*first,
// *first + count). t - origin is taken as a 64-bit unsigned difference where t >= origin (exact: it is below 2^64).
// A segment takes part in bucket b exactly when the range path would take it for the bucket's bounds [lo, hi]
// (k_agg_range: not end < lo, not start > hi) - which, for a malformed segment with end < start whose stream still
// decodes to points, is the one bucket that holds both ends, if any.
__device__ __forceinline__ uint64_t bucket_span(int64_t start, int64_t end, const BucketRequest &r, uint64_t *first) {
    if (end < start) {
        if (end < r.t_lo || start > r.t_hi || end < r.origin) return 0;
        const uint64_t b = ((uint64_t)end - (uint64_t)r.origin) / (uint64_t)r.width;
        if (b >= r.n_buckets || ((uint64_t)start - (uint64_t)r.origin) / (uint64_t)r.width != b) return 0;
        *first = b;
        return 1;
    }
    const int64_t a = start > r.t_lo ? start : r.t_lo;
    const int64_t z = end < r.t_hi ? end : r.t_hi;
    if (a > z || z < r.origin) return 0;
    const uint64_t width = (uint64_t)r.width;
    const uint64_t b_first = a <= r.origin ? 0 : ((uint64_t)a - (uint64_t)r.origin) / width;
    if (b_first >= r.n_buckets) return 0;
    uint64_t b_last = ((uint64_t)z - (uint64_t)r.origin) / width;
    if (b_last >= r.n_buckets) b_last = r.n_buckets - 1;
    *first = b_first;
    return b_last - b_first + 1;
}

// [lo, hi] of bucket b (one that bucket_span returned: origin + b * width is at most a real timestamp, so the
// wrapping arithmetic is exact), ANDed with [t_lo, t_hi]; the bucket's end saturates at INT64_MAX.
__device__ __forceinline__ void bucket_bounds(const BucketRequest &r, uint64_t b, int64_t *lo, int64_t *hi) {
    const int64_t first = (int64_t)((uint64_t)r.origin + b * (uint64_t)r.width);
    const uint64_t room = (uint64_t)INT64_MAX - (uint64_t)first;
    const int64_t last = (uint64_t)r.width - 1 > room ? INT64_MAX : first + (r.width - 1);
    *lo = first > r.t_lo ? first : r.t_lo;
    *hi = last < r.t_hi ? last : r.t_hi;
}

// The last timestamp of bucket n_buckets - 1 (saturating): with [max(t_lo, origin), this] ANDed with [t_lo, t_hi], the
// points any bucket of the request holds.
__device__ __forceinline__ int64_t buckets_last_time(const BucketRequest &r) {
    const uint64_t room = (uint64_t)INT64_MAX - (uint64_t)r.origin; // (origin <= INT64_MAX: the room is exact)
    if (r.n_buckets > room / (uint64_t)r.width) return INT64_MAX;
    return (int64_t)((uint64_t)r.origin + r.n_buckets * (uint64_t)r.width - 1u);
}

// Is segment i's MacaqueV stream - its values (MacaqueV, regular timestamps, no residuals) or the residual tail of a
// PMC-Mean / Swing segment with regular timestamps - aggregated per bucket piece by piece (k_agg_bucket_pieces)
// from the batch's cursor index (piece_base)? The same test as the range path's (mv_range_by_pieces /
// mv_range_tail_by_pieces), evaluated identically by k_agg_bucket_partials, which then leaves those points out.
__device__ __forceinline__ bool bucket_values_by_pieces(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                        const unsigned long long *piece_base) {
    return piece_base && piece_base[i + 1] > piece_base[i] && mv_range_by_pieces(s, i, info);
}
__device__ __forceinline__ bool bucket_tail_by_pieces(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                      const unsigned long long *piece_base) {
    return piece_base && piece_base[i + 1] > piece_base[i] && mv_range_tail_by_pieces(s, i, info);
}

// mdb_buckets.hip: the group ids of host batches (groups[k]: rows[k] ids or nullptr, groups itself may be nullptr) as
// one device array in the context's scratch (*out nullptr: every segment in group 0).
int upload_groups(mdb_ctx *ctx, const uint32_t *const *groups, const uint64_t *rows, uint32_t n_inputs, uint64_t n,
                  const uint32_t **out);

// mdb_buckets.hip: how every host form (a list of host batches, none of them NULL) gets onto the device. The object
// takes the context's lock for as long as it lives; upload() selects the device and makes the list one device batch
// (`transient`: into the context's upload scratch - else an upload the library holds, which gets the cursor index a
// resident batch gets, so that the host and device forms decode the same streams the same way) with its group ids next
// to it; the upload is freed on scope exit. upload_pair(): the operators over two fields - the y list as a batch of its
// own, unless it is the x list (one pointer each, the same pointers), which is then uploaded once.
class UploadedSegments {
public:
    explicit UploadedSegments(mdb_ctx *ctx) : lock_(ctx), ctx_(ctx) {}
    ~UploadedSegments();
    int upload(const mdb_segments *const *inputs, uint32_t n_inputs, const uint32_t *const *group_of_segment,
               bool transient);
    int upload_pair(const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys, uint32_t n_y,
                    const uint32_t *const *group_of_segment_x);
    const mdb_segments *segments() const;
    const mdb_segments *y_segments() const; // (after upload_pair)
    const uint32_t *groups() const { return groups_; }

private:
    CallGuard lock_;
    mdb_ctx *ctx_;
    mdb_segments_owned *dev_ = nullptr, *y_dev_ = nullptr;
    const uint32_t *groups_ = nullptr;
};

} // namespace mdb
