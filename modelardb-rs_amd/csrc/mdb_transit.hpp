// mdb_transit.hpp - transitions between value cells, per date_bin bucket and group (mdb_transit_buckets*): every LINKED
// pair of rows (t0, v0) - (t1, v1) (mdb.h: the rule of mdb_integral_buckets) is one count in
// counts[group][bucket of t1][cell of v0][cell of v1] under the edge list of mdb_hist_buckets; a pair is never cut. The
// product of mdb_change.hpp (the pair-to-bucket rule, the O(1) row ranges) and mdb_hist_dev.hpp (the cell rule, the
// binary searches along a Swing line).
//
// The first part is plain C++ (no HIP type): the request's checks, the walk of a run of rows reduced to keys, the merge
// and the crossings finish. It is shared by the kernel, by the host entry points (mdb_transit_host.cpp) and by the
// check program tests/transit_host, which runs it under the CPU sanitizers. The second part (hipcc only) is the lane
// and what it makes of one segment.
//
// Arithmetic: integers only. A bucket's first instant is formed wrapping (exact for a bucket a real timestamp reaches)
// and its last instant saturates at INT64_MAX (mdb_change.hpp).
#pragma once

#include "mdb_change.hpp"
#include "mdb_hist.hpp"

namespace mdb {

// The buckets [b0, b1) a walk may count into. A pair whose later row lies outside the window is dropped.
struct TransitWindow {
    int64_t origin, width, max_gap;
    uint64_t b0, b1;
};

// A run of rows of one group, fed in row order: the key of the earlier row of every linked pair is held up to the
// later. change_walk_point's bucket logic without the cell: a row between the open bucket's lo and hi needs no
// division, the row behind hi is tried against the next bucket first.
struct TransitWalk {
    uint64_t bucket;
    int64_t lo, hi; // the first and the last instant of the open bucket
    int64_t t_prev;
    int32_t key_prev;
    bool open, have;
};

MDB_INTEGRAL_FN TransitWalk transit_walk_start() { return TransitWalk{0, 0, 0, 0, 0, false, false}; }

// The next row of the run: emit(bucket, from_key, to_key) when it is linked to the row before it and lies in a bucket
// of the window (a malformed stream may step back in time, which links nothing but may land in an earlier bucket).
template <typename Emit>
MDB_INTEGRAL_FN void transit_walk_point(const TransitWindow &w, TransitWalk &walk, int64_t t, int32_t key, Emit emit) {
    if (walk.have && integral_linked(w.max_gap, walk.t_prev, t)) {
        if (walk.open && t >= walk.lo && t <= walk.hi) {
            emit(walk.bucket, walk.key_prev, key);
        } else if (walk.open && t > walk.hi && (uint64_t)t - (uint64_t)walk.hi <= (uint64_t)w.width &&
                   walk.bucket + 1 < w.b1) { // the next bucket (hi < t <= INT64_MAX: hi + 1 does not overflow)
            walk.bucket += 1;
            walk.lo = walk.hi + 1;
            walk.hi = change_bucket_last(walk.lo, w.width);
            emit(walk.bucket, walk.key_prev, key);
        } else if (t >= w.origin) {
            const uint64_t b = ((uint64_t)t - (uint64_t)w.origin) / (uint64_t)w.width;
            if (b >= w.b0 && b < w.b1) {
                walk.open = true;
                walk.bucket = b;
                walk.lo = integral_bucket_start(w.origin, w.width, b); // (<= t, a real timestamp: exact)
                walk.hi = change_bucket_last(walk.lo, w.width);
                emit(b, walk.key_prev, key);
            }
        }
    }
    walk.have = true;
    walk.t_prev = t;
    walk.key_prev = key;
}

// The host-side checks every form makes before it touches the device: those of mdb_change_buckets* and
// mdb_hist_buckets* together; *n_rows = n_groups * n_buckets, with (n_edges + 1)^2 counters each.
inline int transit_request_check(const mdb_transit_request *request, uint32_t n_edges, uint64_t *n_rows) {
    const mdb_bucket_request &b = request->buckets;
    if (b.which_mask != 0) return fail("which_mask must be 0 for mdb_transit_buckets*.");
    if (b.width <= 0) return fail("The bucket width must be positive.");
    if (b.n_groups == 0) return fail("n_groups must be at least 1.");
    if (b.t_lo != INT64_MIN || b.t_hi != INT64_MAX)
        return fail("mdb_transit_buckets* takes no time range: t_lo / t_hi must be INT64_MIN / INT64_MAX.");
    if (request->reserved != 0) return fail("mdb_transit_request.reserved must be 0.");
    if (request->flags != 0) return fail("mdb_transit_request.flags must be 0.");
    if (request->max_gap < 0) return fail("max_gap must not be negative.");
    const unsigned __int128 rows = (unsigned __int128)b.n_groups * b.n_buckets;
    const uint64_t n_cells = (uint64_t)n_edges + 1;
    if (rows * (n_cells * n_cells) > (unsigned __int128)(UINT64_MAX / 16))
        return fail("n_groups * n_buckets * n_cells * n_cells overflows.");
    *n_rows = (uint64_t)rows;
    return 0;
}

inline void transit_merge(uint64_t *into, const uint64_t *from, uint64_t n) {
    for (uint64_t j = 0; j < n; j++) into[j] += from[j];
}

// Per row of n_cells * n_cells counters [from][to] and edge e < n_cells - 1 the pairs that went over it:
//   up[e] = sum of counts[from <= e < to]      down[e] = sum of counts[to <= e < from]
// Edge by edge: moving from e - 1 to e, up gains row e's counters right of the diagonal and loses column e's above it
// (down likewise, mirrored) - n_cells^2 additions per row, in uint64_t (exact wherever the sums fit).
inline void transit_crossings(const uint64_t *counts, uint64_t n_rows, uint32_t n_cells, uint64_t *up, uint64_t *down) {
    if (n_cells < 2) return;
    const uint64_t n = n_cells, n_edges = n - 1;
    for (uint64_t row = 0; row < n_rows; row++) {
        const uint64_t *m = counts + row * n * n;
        uint64_t ups = 0, downs = 0;
        for (uint64_t e = 0; e < n_edges; e++) {
            for (uint64_t c = e + 1; c < n; c++) {
                ups += m[e * n + c];
                downs += m[c * n + e];
            }
            for (uint64_t c = 0; c < e; c++) {
                ups -= m[c * n + e];
                downs -= m[e * n + c];
            }
            up[row * n_edges + e] = ups;
            down[row * n_edges + e] = downs;
        }
    }
}

// mdb_transit.hip: the host batches of the list uploaded and their pairs added to the caller's counters (the request
// and the edges checked, the list not empty). The only step of the host forms that needs the device.
int transit_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                     uint32_t n_inputs, const mdb_transit_request *request, const std::vector<int32_t> &edge_keys,
                     uint64_t n_rows, uint64_t *counts);

} // namespace mdb

#if defined(__HIPCC__)

#include "mdb_hist_dev.hpp"

namespace mdb {

// The lane of the edge list over pairs: the counter [from][to] of one (group, bucket) matrix it is adding to, the pairs
// not added yet, and the key interval of the cell looked up last (as HistLane: a walk searches once per change of
// cell - the later key of a pair is the earlier key of the next, which then lies in the interval).
struct TransitLane {
    const int32_t *edges;     // the edges' keys (LDS)
    uint32_t n_edges;
    unsigned long long *at;   // the counter of the current (row, from, to); nullptr: none yet
    unsigned long long run;   // pairs of that counter not added yet
    int32_t lo, hi;           // the keys of the cell looked up last, closed (lo > hi: none yet)
    uint32_t cell;

    __device__ __forceinline__ uint32_t cell_of(int32_t key) const {
        uint32_t a = 0, b = n_edges;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (edges[mid] <= key) a = mid + 1;
            else b = mid;
        }
        return a;
    }
    __device__ __forceinline__ uint32_t lookup(int32_t key) {
        if (key < lo || key > hi) {
            cell = cell_of(key);
            lo = cell == 0 ? INT32_MIN : edges[cell - 1];
            hi = cell == n_edges ? INT32_MAX : edges[cell] - 1; // (edges[cell] > key: no wrap)
        }
        return cell;
    }
    __device__ __forceinline__ void flush() {
        if (run) atomicAdd(at, run);
        run = 0;
    }
    // n pairs from cell `from` to cell `to` of `matrix` (n_cells * n_cells counters).
    __device__ __forceinline__ void add(unsigned long long *matrix, uint32_t from, uint32_t to, unsigned long long n) {
        unsigned long long *counter = matrix + (uint64_t)from * (n_edges + 1) + to;
        if (counter != at) {
            flush();
            at = counter;
        }
        run += n;
    }
};

// Segment i, whose extent reaches the buckets [b_first, b_first + count), into the matrices row0 + bucket of `cells`
// (row0 = group * n_buckets); the pair with its right neighbour's first row (`heads`) is the segment's own. PMC-Mean on
// regular timestamps: every pair stays in the value's cell, one add per bucket from change_regular_rows. Swing on
// regular timestamps: per bucket the later rows [ka, kb] cover the sorted run ka - 1 .. kb, which is walked cell by cell
// as HistCellsOf::model does - each crossed edge's first row found by one binary search, the pair that ends at it the
// only one off the diagonal. Then only the model's last row, the residual tail and the link are walked. Everything
// else - MacaqueV values, irregular timestamps, a sampling interval the gap rule does not link - is one walk of the rows.
__device__ __forceinline__ void transit_segment(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                const IntegralRequest &q, uint64_t b_first, uint64_t count, uint64_t row0,
                                                TransitLane &lane, unsigned long long *cells, bool neighbour,
                                                const IntegralHead *__restrict__ heads, uint32_t *error) {
    const SegDesc &d = info.desc;
    const BucketRequest &r = q.buckets;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const bool regular = (d.flags & FLAG_REGULAR) != 0;
    const TransitWindow w = {r.origin, r.width, q.max_gap, b_first, b_first + count};
    const uint64_t matrix_cells = ((uint64_t)lane.n_edges + 1) * ((uint64_t)lane.n_edges + 1);
    auto key_of = [](float v) { return total_order_key(__float_as_uint(v)); };
    auto matrix_of = [&](uint64_t b) { return cells + (row0 + b) * matrix_cells; };
    auto pair = [&](uint64_t b, int32_t from_key, int32_t to_key) {
        const uint32_t from = lane.lookup(from_key); // (the interval of the row before: no search)
        lane.add(matrix_of(b), from, lane.lookup(to_key), 1);
    };
    const bool model = regular && type != MDB_MACAQUE_V_ID && d.n_model >= 1;
    const bool closed = model && d.n_model >= 2 && integral_linked(q.max_gap, 0, d.delta);
    if (closed) {
        for (uint64_t b = w.b0; b < w.b1; b++) {
            const int64_t start = integral_bucket_start(r.origin, r.width, b);
            uint32_t ka = 0, kb = 0;
            const uint64_t pairs = change_regular_rows(d.start, d.delta, d.n_model, start, change_bucket_last(start, r.width), &ka, &kb);
            if (pairs == 0) continue;
            unsigned long long *matrix = matrix_of(b);
            if (type == MDB_PMC_MEAN_ID) {
                const uint32_t c = lane.lookup(key_of(d.value));
                lane.add(matrix, c, c, pairs);
                continue;
            }
            // Swing: the rows ka - 1 .. kb (the pair (ka - 1, ka) is this bucket's wherever row ka - 1 lies)
            auto key_at = [&](uint32_t k) { return key_of(swing_value_at(d, k)); };
            auto point_by_point = [&]() {
                int32_t before = key_at(ka - 1);
                for (uint32_t k = ka;; k++) {
                    const int32_t key = key_at(k);
                    pair(b, before, key);
                    before = key;
                    if (k == kb) break;
                }
            };
            const float va = swing_value_at(d, ka - 1), vb = swing_value_at(d, kb);
            if (va != va || vb != vb) { // (as HistCellsOf::model: the run is not known to be sorted)
                point_by_point();
                continue;
            }
            const int32_t key_a = key_of(va), key_b = key_of(vb);
            const uint32_t cb = lane.lookup(key_b), ca = lane.lookup(key_a);
            if (ca == cb) { // (the keys between the ends lie between them)
                lane.add(matrix, ca, ca, pairs);
                continue;
            }
            const uint32_t crossed = ca < cb ? cb - ca : ca - cb;
            const uint32_t steps = 32u - (uint32_t)__clz((uint32_t)pairs); // ceil(log2(rows)), rows = pairs + 1 >= 2
            if ((uint64_t)crossed * steps > pairs + 1) {
                point_by_point();
                continue;
            }
            const bool up = key_a < key_b;
            uint32_t at = ka - 1;
            while (at < kb) {
                const uint32_t c = lane.lookup(key_at(at));
                if (c == cb) {
                    lane.add(matrix, c, c, kb - at);
                    break;
                }
                const int32_t lo = lane.lo, hi = lane.hi;
                // (row kb lies past the cell: the search ends at or before it)
                const uint32_t next = up ? swing_first_past(d, at + 1, kb, [&](int32_t key) { return key > hi; })
                                         : swing_first_past(d, at + 1, kb, [&](int32_t key) { return key < lo; });
                if (next - 1 > at) lane.add(matrix, c, c, next - 1 - at);
                lane.add(matrix, c, lane.lookup(key_at(next)), 1); // the boundary pair: it may skip cells
                at = next;
            }
        }
    }
    const int64_t window_last = change_bucket_last(integral_bucket_start(r.origin, r.width, w.b1 - 1), r.width);
    const IntegralHead head = neighbour ? heads[i + 1] : IntegralHead{0.0f, 0u};
    const int64_t next = neighbour ? s.start_time[i + 1] : 0;
    const int64_t t_last = regular ? (d.n_total > 0 ? trend_time_at(d, d.n_total - 1) : d.start) : s.end_time[i];
    const bool link = neighbour && head.rows > 0 && d.n_total > 0 && integral_linked(q.max_gap, t_last, next);
    TransitWalk walk = transit_walk_start();
    auto point = [&](int64_t t, float v) { transit_walk_point(w, walk, t, key_of(v), pair); };
    const uint32_t n_res = d.n_total - d.n_model;
    if (model) {
        if (n_res > 0 || link) point(trend_time_at(d, d.n_model - 1), d.value);
        if (n_res > 0) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, n_res, true, __float_as_uint(d.value), error,
                             [&](uint32_t k, uint32_t bits) { point(trend_time_at(d, d.n_model + k), __uint_as_float(bits)); });
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
        integral_rows(s, i, info, limit, error, point);
    }
    if (link) point(next, head.value);
}

} // namespace mdb

#endif // __HIPCC__
