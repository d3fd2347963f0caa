// mdb_m4.hpp - M4 downsampling (mdb_m4_buckets*): the first, last, lowest and highest point of every date_bin bucket
// and group, with their timestamps.
//
// The first part is plain C++ (no HIP type): the four selection rules on cells, and the checks of a request. It is
// shared by the kernels, by the host entry points (mdb_m4_host.cpp) and by the check program tests/m4_host, which runs
// it under the CPU sanitizers. The second part (hipcc only) is what one lane makes of one (segment, bucket) pair.
//
// The rules, with key(v) the totalOrder key of mdb_value_filter:
//   first = the smallest (t, key(v))      last = the largest (t, key(v))
//   min   = the smallest (key(v), t)      max  = the largest key(v), among those the smallest t
// Each is a minimum under a total order of the points, so merging is commutative and associative: nothing depends on
// the order of the segments, on how a batch is cut, on the slices, the sort path or the shape of the reduction tree.
// Equal keys are equal bit patterns, so the bytes of a cell are a function of the set of its points alone.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include "mdb_buckets.hpp"
#define MDB_M4_FN __host__ __device__ __forceinline__
#else
#include "mdb_host_side.hpp"
#define MDB_M4_FN inline
#endif

namespace mdb {

MDB_M4_FN int32_t m4_key(float v) {
    uint32_t bits;
    __builtin_memcpy(&bits, &v, 4);
    return (int32_t)(bits ^ ((uint32_t)((int32_t)bits >> 31) & 0x7fffffffu));
}

// A pair's (or a run's) four points in scratch: mdb_m4_cell padded to 64 bytes, so that a record is four aligned
// 16-byte words (read and written as such, m4_load / m4_store) and never straddles a 64-byte sector.
struct alignas(16) M4Partial {
    int64_t count;
    int64_t t_first, t_last, t_min, t_max;
    float v_first, v_last, v_min, v_max;
    uint32_t unused[2];
};
static_assert(sizeof(M4Partial) == 64, "records are laid out in scratch by this size");

// Does the point (t, key) come before (t0, key0) when compared by time first / by key first? Branch-free on purpose
// (| and &, then selects below): the four updates of a merge are conditional moves, not divergent branches. (Written as
// `if (t < t0 || (t == t0 && key < key0)) { ... }`, the gfx950 code hipcc made for k_m4_tree kept the old value on a tie
// of the timestamps; the tests with several series in one group caught it.)
MDB_M4_FN bool m4_before(int64_t t, int32_t key, int64_t t0, int32_t key0) {
    return (t < t0) | ((t == t0) & (key < key0));
}
MDB_M4_FN bool m4_after(int64_t t, int32_t key, int64_t t0, int32_t key0) {
    return (t > t0) | ((t == t0) & (key > key0));
}

// The points of `from` added to those of `into`: each of the four by its rule. An empty `from` changes nothing; an
// empty `into` (count 0: no other member is read) takes every member of `from`. A, B: mdb_m4_cell or M4Partial (the
// same members).
template <typename A, typename B> MDB_M4_FN void m4_merge(A &into, const B &from) {
    if (from.count == 0) return;
    if (into.count == 0) {
        into.count = from.count;
        into.t_first = from.t_first, into.t_last = from.t_last, into.t_min = from.t_min, into.t_max = from.t_max;
        into.v_first = from.v_first, into.v_last = from.v_last, into.v_min = from.v_min, into.v_max = from.v_max;
        return;
    }
    const bool first = m4_before(from.t_first, m4_key(from.v_first), into.t_first, m4_key(into.v_first));
    const bool last = m4_after(from.t_last, m4_key(from.v_last), into.t_last, m4_key(into.v_last));
    const int32_t low = m4_key(from.v_min), into_low = m4_key(into.v_min);
    const int32_t high = m4_key(from.v_max), into_high = m4_key(into.v_max);
    const bool lower = (low < into_low) | ((low == into_low) & (from.t_min < into.t_min));
    const bool higher = (high > into_high) | ((high == into_high) & (from.t_max < into.t_max));
    into.t_first = first ? from.t_first : into.t_first, into.v_first = first ? from.v_first : into.v_first;
    into.t_last = last ? from.t_last : into.t_last, into.v_last = last ? from.v_last : into.v_last;
    into.t_min = lower ? from.t_min : into.t_min, into.v_min = lower ? from.v_min : into.v_min;
    into.t_max = higher ? from.t_max : into.t_max, into.v_max = higher ? from.v_max : into.v_max;
    into.count += from.count;
}

// One more point: the merge of a cell that holds just that point.
template <typename T> MDB_M4_FN void m4_point(T &c, int64_t t, float v) {
    struct {
        int64_t count, t_first, t_last, t_min, t_max;
        float v_first, v_last, v_min, v_max;
    } one = {1, t, t, t, t, v, v, v, v};
    m4_merge(c, one);
}

// The host-side checks every form makes before it touches the device: those of mdb_agg_buckets*, and which_mask == 0.
inline int m4_request_check(const mdb_bucket_request *request, uint64_t *n_cells) {
    if (request->which_mask != 0) return fail("which_mask must be 0 for mdb_m4_buckets*.");
    if (request->width <= 0) return fail("The bucket width must be positive.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    const unsigned __int128 cells = (unsigned __int128)request->n_groups * request->n_buckets;
    if (cells * sizeof(mdb_m4_cell) > (unsigned __int128)UINT64_MAX) return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// mdb_m4.hip: the host batches of the list uploaded and folded into the caller's cells (the request checked, the
// list not empty). The only step of the host forms that needs the device.
int m4_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                uint32_t n_inputs, const mdb_bucket_request *request, uint64_t n_cells, mdb_m4_cell *inout);

} // namespace mdb

#if defined(__HIPCC__)

namespace mdb {

__device__ __forceinline__ void m4_store(M4Partial *to, const M4Partial &value) {
    uint4 words[4];
    __builtin_memcpy(words, &value, 64);
    uint4 *out = reinterpret_cast<uint4 *>(to);
    out[0] = words[0], out[1] = words[1], out[2] = words[2], out[3] = words[3];
}
__device__ __forceinline__ M4Partial m4_load(const M4Partial *from) {
    const uint4 *in = reinterpret_cast<const uint4 *>(from);
    const uint4 words[4] = {in[0], in[1], in[2], in[3]};
    M4Partial value;
    __builtin_memcpy(&value, words, 64);
    return value;
}
__device__ __forceinline__ M4Partial m4_empty() { return M4Partial{0, 0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, {0u, 0u}}; }

__device__ __forceinline__ int64_t m4_time_at(const SegDesc &d, uint32_t k) {
    return d.start + (int64_t)((uint64_t)k * (uint64_t)d.delta);
}

// The model points [a, b] of a PMC-Mean or Swing segment with regular timestamps. PMC-Mean: point a is first, min and
// max, point b last. Swing: the keys are sorted along k (model_run, mdb_filter.hpp), so the ends are first and last,
// the extreme on the side of a is point a, and the other extreme has b's value at the earliest k that already has b's
// key - several consecutive points can round to one f32 - found by one binary search with exact evaluations. An end
// that evaluates to NaN: every point is tested (the run is not known to be sorted). The stored min_value / max_value
// are not used.
__device__ __forceinline__ void m4_model_points(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, M4Partial &acc) {
    auto point_by_point = [&]() {
        for (uint32_t k = a;; k++) {
            const int64_t t = m4_time_at(d, k);
            m4_point(acc, t, model_value_at(d, type, t));
            if (k == b) break;
        }
    };
    if (a == b || d.delta <= 0) return point_by_point(); // (delta <= 0: the two points of a segment with end <= start)
    const int64_t ta = m4_time_at(d, a), tb = m4_time_at(d, b);
    M4Partial run = m4_empty();
    run.count = (int64_t)(b - a) + 1;
    run.t_first = ta, run.t_last = tb;
    if (type == MDB_PMC_MEAN_ID) {
        run.t_min = run.t_max = ta;
        run.v_first = run.v_last = run.v_min = run.v_max = d.value;
    } else {
        const float va = swing_value_at(d, a), vb = swing_value_at(d, b);
        if (va != va || vb != vb) return point_by_point();
        const int32_t ka = m4_key(va), kb = m4_key(vb);
        run.v_first = va, run.v_last = vb;
        const bool up = ka <= kb;
        // (b itself has the key: the search over [a, b) returns b if no earlier point has it)
        const uint32_t k_far = ka == kb ? a
                               : up     ? swing_first_past(d, a, b, [&](int32_t key) { return key >= kb; })
                                        : swing_first_past(d, a, b, [&](int32_t key) { return key <= kb; });
        const int64_t t_far = m4_time_at(d, k_far);
        run.t_min = up ? ta : t_far, run.v_min = up ? va : vb;
        run.t_max = up ? t_far : ta, run.v_max = up ? vb : va;
    }
    m4_merge(acc, run);
}

// The points of a PMC-Mean or Swing segment with regular timestamps inside [lo, hi]: the model's in closed form, the
// residual tail's decoded (not when the tail is k_m4_pieces').
__device__ __forceinline__ void m4_regular_pair(const DevSegments &s, uint64_t i, const SegInfo &info, int64_t lo,
                                                int64_t hi, M4Partial &acc, uint32_t *error, bool tail_by_pieces) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const uint32_t n_res = d.n_total - d.n_model;
    uint32_t k_lo = 0, k_hi = 0;
    if (!regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi)) return;
    if (k_lo < d.n_model) m4_model_points(d, type, k_lo, min(k_hi, d.n_model - 1), acc);
    if (n_res > 0 && k_hi >= d.n_model && !tail_by_pieces) {
        const uint4 vr = s.residuals.views[i];
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, k_hi - d.n_model + 1, true, __float_as_uint(d.value),
                         error, [&](uint32_t k, uint32_t bits) {
                             const uint32_t index = d.n_model + k;
                             if (index >= k_lo) m4_point(acc, m4_time_at(d, index), __uint_as_float(bits));
                         });
    }
}

// Where pass 1 of a stream leaves slot j's index interval [x, y] of points (x > y: none): the record's first 8 bytes.
__device__ __forceinline__ uint2 *m4_interval(M4Partial *slot) { return reinterpret_cast<uint2 *>(&slot->count); }

// Pass 2 and 3 over the slots [j0, j1) of a segment whose points are a bit stream, each slot holding its index
// interval (ascending, disjoint): the values are decoded once, up to point `needed` - 1, each into the slot whose
// interval holds it, and every slot is overwritten with its record. Regular timestamps give every point its time;
// for irregular ones the records hold point INDICES first (the rules on (index, key) choose the same points while the
// timestamps ascend), and one more walk of the timestamp stream turns the recorded indices into timestamps.
__device__ __forceinline__ void m4_stream_decode(const DevSegments &s, uint64_t i, const SegInfo &info, uint64_t j0,
                                                 uint64_t j1, uint64_t p0, M4Partial *__restrict__ out, uint32_t needed,
                                                 uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint32_t n_res = d.n_total - d.n_model;
    const bool regular = (d.flags & FLAG_REGULAR) != 0;
    uint64_t j = j0;
    uint2 current = *m4_interval(&out[j - p0]);
    M4Partial acc = m4_empty();
    auto flush = [&]() {
        m4_store(&out[j - p0], acc);
        acc = m4_empty();
        j++;
        if (j < j1) current = *m4_interval(&out[j - p0]);
    };
    auto visit = [&](uint32_t k, float v) {
        while (j < j1 && k > current.y) flush();
        if (j < j1 && k >= current.x) m4_point(acc, regular ? m4_time_at(d, k) : (int64_t)k, v);
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
    if (regular || needed == 0) return;

    // Pass 3: the slots' recorded indices (first <= min, max <= last, ascending from slot to slot) become timestamps.
    uint64_t slot = j0;
    M4Partial record = m4_empty();
    uint32_t i_first = 0, i_last = 0, i_min = 0, i_max = 0;
    auto open = [&]() { // the next slot that holds points, if any
        for (; slot < j1; slot++) {
            record = m4_load(&out[slot - p0]);
            if (record.count > 0) break;
        }
        i_first = (uint32_t)record.t_first, i_last = (uint32_t)record.t_last;
        i_min = (uint32_t)record.t_min, i_max = (uint32_t)record.t_max;
    };
    open();
    if (slot >= j1) return;
    const uint4 vt = s.timestamps.views[i];
    decode_irregular_timestamps(view_data(s.timestamps, i, vt), vt.x, d.start, end, needed, error,
                                [&](uint32_t k, int64_t t) {
                                    if (slot >= j1) return;
                                    if (k == i_first) record.t_first = t;
                                    if (k == i_min) record.t_min = t;
                                    if (k == i_max) record.t_max = t;
                                    if (k == i_last) {
                                        record.t_last = t;
                                        m4_store(&out[slot - p0], record);
                                        slot++;
                                        open();
                                    }
                                });
}

// The pairs of a segment whose points are a bit stream (MacaqueV values, irregular timestamps): slots [j0, j1) of the
// slice, buckets b_first + (j - off), as bucket_stream_partials (mdb_buckets.hip) - pass 1 leaves each slot's index
// interval, m4_stream_decode does the rest. Returns false when the timestamps turn out not to be sorted (a malformed
// stream): the caller then goes pair by pair (m4_unsorted_pair).
__device__ __forceinline__ bool m4_stream_partials(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                   const BucketRequest &r, uint64_t off, uint64_t b_first, uint64_t j0,
                                                   uint64_t j1, uint64_t p0, M4Partial *__restrict__ out, uint32_t *error) {
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
            *m4_interval(&out[j - p0]) = make_uint2(k_lo, k_hi);
        }
    } else {
        for (uint64_t j = j0; j < j1; j++) *m4_interval(&out[j - p0]) = make_uint2(1, 0);
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
                                            if (slot != ~0ull) *m4_interval(&out[slot - p0]) = make_uint2(k_lo, k_hi);
                                            slot = j;
                                            k_lo = k;
                                        }
                                        k_hi = k;
                                    });
        if (!sorted) return false;
        if (slot != ~0ull) {
            *m4_interval(&out[slot - p0]) = make_uint2(k_lo, k_hi);
            needed = k_hi + 1;
        }
    }
    m4_stream_decode(s, i, info, j0, j1, p0, out, needed, error);
    return true;
}

// One pair [lo, hi] of a segment with irregular timestamps that are not sorted (a malformed stream), into *slot: the
// points the range aggregate counts for the same bounds (segment_range, mdb_agg_dev.hpp). A model without residuals:
// every point is tested with its own timestamp. Values in a bit stream: the indices between the first and the last
// timestamp inside [lo, hi], chosen among by (index, key) and reported with their own timestamps.
__device__ __forceinline__ void m4_unsorted_pair(const DevSegments &s, uint64_t i, const SegInfo &info, int64_t lo,
                                                 int64_t hi, uint64_t j, uint64_t p0, M4Partial *__restrict__ out,
                                                 uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint4 vt = s.timestamps.views[i];
    const uint8_t *ts_bytes = view_data(s.timestamps, i, vt);
    if (type != MDB_MACAQUE_V_ID && d.n_total == d.n_model) {
        M4Partial acc = m4_empty();
        if (!(end < lo || d.start > hi))
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t, int64_t t) {
                if (t >= lo && t <= hi) m4_point(acc, t, model_value_at(d, type, t));
            });
        m4_store(&out[j - p0], acc);
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
    *m4_interval(&out[j - p0]) = any ? make_uint2(k_lo, k_hi) : make_uint2(1, 0);
    m4_stream_decode(s, i, info, j, j + 1, p0, out, any ? k_hi + 1 : 0, error);
}

} // namespace mdb

#endif // __HIPCC__
