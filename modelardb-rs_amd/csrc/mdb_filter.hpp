// mdb_filter.hpp - the value predicate of mdb_value_filter (mdb_format.h) on the device, the two selectors of
// segment_range (mdb_agg_dev.hpp) that do not look at rows, and the run of passing points of a model: shared by the
// filtered aggregates (mdb_agg.hip, mdb_buckets.hip), the filtered grid (mdb_filter.hip) and the row masks.
#pragma once

#include "mdb_segment_dev.hpp"

#include <climits>
#include <cstring>

namespace mdb {

// IEEE 754 totalOrder as a signed integer: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN.
__host__ __device__ __forceinline__ int32_t total_order_key(uint32_t bits) {
    return (int32_t)(bits ^ ((uint32_t)((int32_t)bits >> 31) & 0x7fffffffu));
}

struct RangeAcc; // (mdb_agg_dev.hpp)

// A SELECTOR says which points of a segment the walk of mdb_agg_dev.hpp (segment_range) takes. It answers two
// questions: counts(v, row) - does the point of value v, the row-th of the segment's points inside the time range,
// count? - and model(d, type, a, b, row_a, acc): what the model points [a, b] of a PMC-Mean or Swing segment with
// regular timestamps (point a is row row_a) add to acc. by_row: does it look at rows at all? Three of them: AllValues
// and ValueKeys here, SegmentRows in mdb_mask.hpp. (model() of the two here: mdb_agg_dev.hpp, behind the closed form)

// Every point counts (the range calls, the default of segment_range).
struct AllValues {
    static constexpr bool by_row = false;
    __device__ __forceinline__ bool counts(float, uint64_t) const { return true; }
    __device__ __forceinline__ void model(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, uint64_t row_a,
                                          RangeAcc &acc) const;
};

// The value bounds folded into one closed interval of keys [lo, hi] (lo > hi: nothing passes).
struct ValueKeys {
    static constexpr bool by_row = false;
    int32_t lo;
    int32_t hi;
    __device__ __forceinline__ bool key_passes(int32_t key) const { return key >= lo && key <= hi; }
    __device__ __forceinline__ bool pass(float v) const { return key_passes(total_order_key(__float_as_uint(v))); }
    __device__ __forceinline__ bool counts(float v, uint64_t) const { return pass(v); }
    __device__ __forceinline__ void model(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, uint64_t row_a,
                                          RangeAcc &acc) const;
};

// Host: the flags folded into closed key bounds (an open end moves by one key; at the ±NaN ends there is no key
// beyond, and the interval is empty). What every entry point with a filter begins with: 0, or 1 and the message for
// unknown flag bits or reserved != 0.
inline int value_keys_fold(const mdb_value_filter *filter, ValueKeys *out) {
    const mdb_value_filter &f = *filter;
    const uint32_t known = MDB_VALUE_LO_OPEN | MDB_VALUE_HI_OPEN | MDB_VALUE_NO_LO | MDB_VALUE_NO_HI;
    if ((f.flags & ~known) != 0 || f.reserved != 0)
        return fail("The value filter has unknown flag bits or a reserved field that is not 0.");
    uint32_t lo_bits, hi_bits;
    std::memcpy(&lo_bits, &f.v_lo, 4);
    std::memcpy(&hi_bits, &f.v_hi, 4);
    int64_t lo = (f.flags & MDB_VALUE_NO_LO) ? (int64_t)INT32_MIN : (int64_t)total_order_key(lo_bits);
    int64_t hi = (f.flags & MDB_VALUE_NO_HI) ? (int64_t)INT32_MAX : (int64_t)total_order_key(hi_bits);
    if (!(f.flags & MDB_VALUE_NO_LO) && (f.flags & MDB_VALUE_LO_OPEN)) lo += 1; // (INT32_MAX + 1: empty)
    if (!(f.flags & MDB_VALUE_NO_HI) && (f.flags & MDB_VALUE_HI_OPEN)) hi -= 1; // (INT32_MIN - 1: empty)
    if (lo > hi || lo > INT32_MAX || hi < INT32_MIN) {
        out->lo = INT32_MAX;
        out->hi = INT32_MIN;
    } else {
        out->lo = (int32_t)lo;
        out->hi = (int32_t)hi;
    }
    return 0;
}

// What a value predicate makes of the model points k in [a, b] of a PMC-Mean or Swing segment with regular
// timestamps start + k * delta.
enum : int { RUN_NONE = 0, RUN_INTERVAL = 1, RUN_POINTS = 2 };

// RUN_NONE: no point passes. RUN_INTERVAL: exactly the points [*ra, *rb] pass. RUN_POINTS: test every point (an end
// evaluates to NaN). PMC-Mean is one value. Swing's points v(k) = (float)(slope * (double)t_k + intercept) are
// monotone in k in IEEE order (a product with a fixed factor, a sum with a fixed addend and the cast to f32 all round
// monotonically), and also in totalOrder: the only IEEE ties totalOrder splits are -0.0 and +0.0, and in
// round-to-nearest an exact-zero sum is +0.0 unless both addends are -0.0 - which for slope * t needs a zero slope
// or t = 0 and then orders the zeros along the line's direction (+0 on the side where slope * t is +0) - while a
// value that rounds to zero in the cast keeps the sign of its side of zero. So the run of keys is sorted (its
// direction given by the two ends) and the passing points are one interval, found by two binary searches over k
// with exact evaluations: at most 2 * ceil(log2(b - a + 2)) evaluations. The stored min_value / max_value are not
// used: at epoch-scale timestamps the evaluated points can round past them.
// Point k of a Swing segment with regular timestamps, as grid() rebuilds it.
__device__ __forceinline__ float swing_value_at(const SegDesc &d, uint32_t k) {
    const int64_t t = d.start + (int64_t)((uint64_t)k * (uint64_t)d.delta);
    return (float)(d.slope * (double)t + d.intercept);
}

// The first k in [lo, hi) whose key is `past` (past is false ... false, true ... true along k, the keys of a Swing
// segment being sorted; hi if none): a binary search with exact evaluations. Shared with the histograms (mdb_hist.hip).
template <typename Past>
__device__ __forceinline__ uint32_t swing_first_past(const SegDesc &d, uint32_t lo, uint32_t hi, const Past &past) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (past(total_order_key(__float_as_uint(swing_value_at(d, mid))))) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

template <typename Pred>
__device__ __forceinline__ int model_run(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, const Pred &pred,
                                         uint32_t *ra, uint32_t *rb) {
    if (type == MDB_PMC_MEAN_ID) {
        if (!pred.pass(d.value)) return RUN_NONE;
        *ra = a;
        *rb = b;
        return RUN_INTERVAL;
    }
    const float va = swing_value_at(d, a), vb = swing_value_at(d, b);
    if (va != va || vb != vb) return RUN_POINTS;
    const int32_t ka = total_order_key(__float_as_uint(va)), kb = total_order_key(__float_as_uint(vb));
    if (pred.key_passes(ka) && pred.key_passes(kb)) {
        *ra = a;
        *rb = b;
        return RUN_INTERVAL;
    }
    if ((ka < pred.lo && kb < pred.lo) || (ka > pred.hi && kb > pred.hi)) return RUN_NONE;
    const bool up = ka <= kb;
    // The first k in [a, b + 1) for which `past` holds (past is false ... false, true ... true along k).
    auto first = [&](auto past) { return swing_first_past(d, a, b + 1, past); };
    const uint32_t s = up ? first([&](int32_t key) { return key >= pred.lo; }) : first([&](int32_t key) { return key <= pred.hi; });
    const uint32_t e = up ? first([&](int32_t key) { return key > pred.hi; }) : first([&](int32_t key) { return key < pred.lo; });
    if (s >= e) return RUN_NONE;
    *ra = s;
    *rb = e - 1;
    return RUN_INTERVAL;
}

// mdb_agg.hip: the filtered aggregates of a batch in HBM folded into *inout (the lock held, the device set).
int agg_filter_run(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const ValueKeys &keys,
                   uint32_t which_mask, mdb_agg_state *inout);

// mdb_grid.hip: the range grid of a batch in HBM (the lock held, the device set) - its prepass alone (the point
// count, the metrics and, if rows_per_segment is given, the rows of every segment), or the points themselves.
int grid_range_plan(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, uint64_t *total,
                    mdb_grid_metrics *metrics, uint32_t *rows_per_segment);
int grid_batch_dev_locked(mdb_ctx *ctx, const mdb_segments *in, TimeRange range, int64_t *out_ts, float *out_val,
                          uint32_t *out_rows, uint64_t cap, uint64_t *n_out, mdb_grid_metrics *metrics);

} // namespace mdb
