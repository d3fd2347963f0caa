// mdb_sample.hpp - the value of a series at regular instants (mdb_sample_at*): gap-fill, last observation carried
// forward, interpolation. Per instant origin + k * width and group one mdb_sample_cell {count, sum}: the rows that lie
// on the instant and, under LINEAR and STEP, the LINKED intervals (mdb.h: same group, time moving forward, the gap
// within max_gap) that contain it.
//
// The first part is plain C++ (no HIP type): which instants a closed extent or an open interval contains, f(T) for the
// three methods, the cell add, the walk of a run of rows over a window of instants and the request's checks. It is
// shared by the kernels, by the host entry points (mdb_sample_host.cpp) and by the check program tests/sample_host,
// which runs it under the CPU sanitizers. The second part (hipcc only) is what a lane makes of a pair and of a segment.
//
// Arithmetic. Every time difference is formed in uint64_t (it is below 2^64 for any two int64 instants) and converted
// to f64 once. Instant k is formed wrapping, origin + k * width, and only for a k found between two real timestamps,
// for which it is exact: an instant no timestamp can reach is never formed. A cell that has received nothing takes its
// first contribution whole, so a cell with count == 1 holds that contribution bit for bit (a -0.0 and a NaN's payload
// included).
#pragma once

#if defined(__HIPCC__)
#include "mdb_integral.hpp"
#define MDB_SAMPLE_FN __host__ __device__ __forceinline__
#else
#include "mdb_host_side.hpp"
#define MDB_SAMPLE_FN inline
#endif

#include <cstdint>

namespace mdb {

// (integral_linked of mdb_integral.hpp, which plain C++ does not include here: the same rule, letter for letter)
MDB_SAMPLE_FN bool sample_linked(int64_t max_gap, int64_t t_prev, int64_t t) {
    return t > t_prev && (uint64_t)t - (uint64_t)t_prev <= (uint64_t)max_gap;
}

MDB_SAMPLE_FN int64_t sample_instant(int64_t origin, int64_t width, uint64_t k) {
    return (int64_t)((uint64_t)origin + k * (uint64_t)width);
}

// The instants k < n inside the closed extent [a, e]: [*first, *first + count). a - origin and e - origin are taken
// where they are not negative, as 64-bit unsigned differences.
MDB_SAMPLE_FN uint64_t sample_instants_closed(int64_t origin, int64_t width, uint64_t n, int64_t a, int64_t e,
                                              uint64_t *first) {
    if (n == 0 || e < a || e < origin) return 0;
    const uint64_t w = (uint64_t)width;
    uint64_t k0 = 0;
    if (a > origin) {
        const uint64_t d = (uint64_t)a - (uint64_t)origin;
        k0 = d / w + (d % w != 0); // (a remainder means w >= 2: the quotient is at most 2^63)
    }
    if (k0 >= n) return 0;
    uint64_t k1 = ((uint64_t)e - (uint64_t)origin) / w;
    if (k1 >= n) k1 = n - 1;
    if (k1 < k0) return 0;
    *first = k0;
    return k1 - k0 + 1;
}

// The instants k < n strictly inside (t0, t1), t1 > t0.
MDB_SAMPLE_FN uint64_t sample_instants_open(int64_t origin, int64_t width, uint64_t n, int64_t t0, int64_t t1,
                                            uint64_t *first) {
    if (t1 <= t0 || (uint64_t)t1 - (uint64_t)t0 < 2) return 0;
    return sample_instants_closed(origin, width, n, t0 + 1, t1 - 1, first); // (t0 < t1: neither step overflows)
}

// Does t lie on an instant k < n?
MDB_SAMPLE_FN bool sample_on_instant(int64_t origin, int64_t width, uint64_t n, int64_t t, uint64_t *k) {
    if (t < origin) return false;
    const uint64_t d = (uint64_t)t - (uint64_t)origin, w = (uint64_t)width;
    if (d % w != 0 || d / w >= n) return false;
    *k = d / w;
    return true;
}

// f(T) on the linked interval (t0, v0) - (t1, v1), t0 < T < t1, under LINEAR or STEP.
MDB_SAMPLE_FN double sample_value(uint32_t method, int64_t t0, float v0, int64_t t1, float v1, int64_t at) {
    if (method == MDB_SAMPLE_STEP || v0 == v1) return (double)v0;
    const double part = (double)((uint64_t)at - (uint64_t)t0), whole = (double)((uint64_t)t1 - (uint64_t)t0);
    return (double)v0 + ((double)v1 - (double)v0) * (part / whole);
}

MDB_SAMPLE_FN void sample_cell_add(mdb_sample_cell &into, const mdb_sample_cell &from) {
    if (from.count == 0) return;
    if (into.count == 0) {
        into = from;
        return;
    }
    into.count += from.count;
    into.sum += from.sum;
}

MDB_SAMPLE_FN void sample_cell_contribute(mdb_sample_cell &into, double value) {
    sample_cell_add(into, mdb_sample_cell{1, value});
}

// The instants [k0, k1) a walk may write, cells[k - k0]: every one of them lies inside the segment's extent, so it is
// exact when formed, and t_lo / t_hi are the first and the last of them. What a walk finds outside is dropped.
struct SampleWindow {
    int64_t origin, width, max_gap;
    uint64_t k0, k1;
    int64_t t_lo, t_hi;
    uint32_t method;
    mdb_sample_cell *cells;
};

MDB_SAMPLE_FN SampleWindow sample_window(int64_t origin, int64_t width, int64_t max_gap, uint32_t method, uint64_t k0,
                                         uint64_t k1, mdb_sample_cell *cells) {
    SampleWindow w = {origin, width, max_gap, k0, k1, 0, 0, method, cells};
    if (k0 < k1) {
        w.t_lo = sample_instant(origin, width, k0);
        w.t_hi = sample_instant(origin, width, k1 - 1);
    }
    return w;
}

// A run of rows of one group, fed row by row in row order. Where a row lies among the instants is found by one
// division, never by a cursor that moves along with the rows: a malformed stream that steps back in time links nothing
// and lands in no cell outside the window.
struct SampleWalk {
    int64_t t_prev;
    float v_prev;
    bool have;
};

MDB_SAMPLE_FN SampleWalk sample_walk_start() { return SampleWalk{0, 0.0f, false}; }

// The row (t, v): ADDED to the cell of the instant it lies on.
MDB_SAMPLE_FN void sample_walk_row(const SampleWindow &w, int64_t t, float v) {
    if (w.k0 >= w.k1 || t < w.t_lo || t > w.t_hi) return;
    const uint64_t d = (uint64_t)t - (uint64_t)w.origin, width = (uint64_t)w.width; // (t >= t_lo >= origin)
    if (d % width != 0) return;
    const uint64_t k = d / width; // (t_lo <= t <= t_hi: k0 <= k < k1)
    sample_cell_contribute(w.cells[k - w.k0], (double)v);
}

// The linked interval (t0, v0) - (t1, v1), t1 > t0: f(T) ADDED to the cell of every instant strictly inside it.
MDB_SAMPLE_FN void sample_walk_interval(const SampleWindow &w, int64_t t0, float v0, int64_t t1, float v1) {
    if (w.k0 >= w.k1 || t1 <= w.t_lo || t0 >= w.t_hi) return;
    uint64_t first = 0;
    // (the instants are looked for below k1 only: the count is then below the window's size plus what lies before it)
    const uint64_t count = sample_instants_open(w.origin, w.width, w.k1, t0, t1, &first);
    if (count == 0) return;
    const uint64_t a = first > w.k0 ? first : w.k0, e = first + count; // (e <= k1)
    for (uint64_t k = a; k < e; k++)
        sample_cell_contribute(w.cells[k - w.k0],
                               sample_value(w.method, t0, v0, t1, v1, sample_instant(w.origin, w.width, k)));
}

// The next row of the run; `row`: the row itself contributes (false: another lane has taken it).
MDB_SAMPLE_FN void sample_walk_point(const SampleWindow &w, SampleWalk &walk, int64_t t, float v, bool row) {
    if (walk.have && w.method != MDB_SAMPLE_EXACT && sample_linked(w.max_gap, walk.t_prev, t))
        sample_walk_interval(w, walk.t_prev, walk.v_prev, t, v);
    if (row) sample_walk_row(w, t, v);
    walk.have = true;
    walk.t_prev = t;
    walk.v_prev = v;
}

// The host-side checks every form makes before it touches the device.
inline int sample_request_check(const mdb_sample_request *request, uint64_t *n_cells) {
    const mdb_bucket_request &b = request->instants;
    if (b.which_mask != 0) return fail("which_mask must be 0 for mdb_sample_at*.");
    if (b.width <= 0) return fail("The width between two instants must be positive.");
    if (b.n_groups == 0) return fail("n_groups must be at least 1.");
    if (b.t_lo != INT64_MIN || b.t_hi != INT64_MAX)
        return fail("mdb_sample_at* takes no time range: t_lo / t_hi must be INT64_MIN / INT64_MAX.");
    if (request->method != MDB_SAMPLE_LINEAR && request->method != MDB_SAMPLE_STEP && request->method != MDB_SAMPLE_EXACT)
        return fail("Unknown method: MDB_SAMPLE_LINEAR, MDB_SAMPLE_STEP or MDB_SAMPLE_EXACT.");
    if (request->flags != 0) return fail("mdb_sample_request.flags must be 0.");
    if (request->max_gap < 0) return fail("max_gap must not be negative.");
    const unsigned __int128 cells = (unsigned __int128)b.n_groups * b.n_buckets;
    if (cells * sizeof(mdb_sample_cell) > (unsigned __int128)UINT64_MAX) return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// mdb_sample.hip: the host batches of the list uploaded and sampled into the caller's cells (the request checked, the
// list not empty). The only step of the host forms that needs the device.
int sample_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                    uint32_t n_inputs, const mdb_sample_request *request, uint64_t n_cells, mdb_sample_cell *inout);

} // namespace mdb

#if defined(__HIPCC__)

namespace mdb {

struct SampleRequest { // what the kernels take: the instants (no time range, which_mask 0), the gap rule, the method
    BucketRequest instants;
    int64_t max_gap;
    uint32_t method;
};

// The last instant that is segment i's: the one before its right neighbour's first row when the two are linked by the
// segments' own times - the row at the neighbour's start is the neighbour's, the interval before it is this segment's
// - else its end_time.
__device__ __forceinline__ int64_t sample_extent_end(const DevSegments &s, const uint32_t *groups, uint64_t i,
                                                     int64_t max_gap) {
    const int64_t reach = integral_extent_end(s, groups, i, max_gap), end = s.end_time[i];
    return reach != end ? reach - 1 : end; // (reach > end when linked)
}

__device__ __forceinline__ uint64_t sample_span(const DevSegments &s, const uint32_t *groups, uint64_t i,
                                                const SampleRequest &q, uint64_t *first) {
    const BucketRequest &r = q.instants;
    return sample_instants_closed(r.origin, r.width, r.n_buckets, s.start_time[i],
                                  sample_extent_end(s, groups, i, q.max_gap), first);
}

// Does k_sample_model_pairs take the model rows of this (well-formed) segment in closed form? PMC-Mean or Swing whose
// rows lie at start + k * delta, delta > 0. Both kernels ask this, of the same descriptor.
__device__ __forceinline__ bool sample_closed(const SegDesc &d) {
    return (d.flags & FLAG_REGULAR) != 0 && (d.flags & FLAG_TYPE_MASK) != MDB_MACAQUE_V_ID && d.n_model >= 1 && d.delta > 0;
}

// What the model rows [0, n_model) of a closed segment give the instant `at`: on a row, the row; between two rows
// that the gap rule links, f(at) from the two; nothing behind the model's last row.
__device__ __forceinline__ mdb_sample_cell sample_model_pair(const SegDesc &d, const SampleRequest &q, int64_t at) {
    mdb_sample_cell cell = {0, 0.0};
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    if (at < d.start || at > trend_time_at(d, d.n_model - 1)) return cell;
    const uint64_t off = (uint64_t)at - (uint64_t)d.start, step = (uint64_t)d.delta;
    const uint32_t k = (uint32_t)(off / step);
    if (off % step == 0) {
        cell.count = 1;
        cell.sum = (double)model_value_at(d, type, at);
    } else if (q.method != MDB_SAMPLE_EXACT && integral_linked(q.max_gap, 0, d.delta)) {
        const int64_t t0 = trend_time_at(d, k), t1 = trend_time_at(d, k + 1); // (k + 1 <= n_model - 1)
        cell.count = 1;
        cell.sum = sample_value(q.method, t0, model_value_at(d, type, t0), t1, model_value_at(d, type, t1), at);
    }
    return cell;
}

// What is left of segment i behind k_sample_model_pairs, ADDED into slots [j0, j1) of the slice (slot j: instant
// k_first + (j - off)): every row and interval of a segment that is not closed; of a closed one the residual tail and
// the interval between the model's last row and the tail's first; and the link to the right neighbour (same group;
// `head` its first row), which is this segment's. One walk of the rows.
__device__ __forceinline__ void sample_segment_walk(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                    const SampleRequest &q, uint64_t off, uint64_t k_first, uint64_t j0,
                                                    uint64_t j1, uint64_t p0, mdb_sample_cell *__restrict__ out,
                                                    bool neighbour, const IntegralHead *__restrict__ heads,
                                                    uint32_t *error) {
    const SegDesc &d = info.desc;
    const BucketRequest &r = q.instants;
    const bool regular = (d.flags & FLAG_REGULAR) != 0;
    const bool closed = sample_closed(d);
    const uint32_t n_res = d.n_total - d.n_model;
    const bool between = q.method != MDB_SAMPLE_EXACT;
    // The link is walked when the rows' own rule may link it; the last row's time is arithmetic on regular timestamps
    // and end_time on irregular ones (the stream does not store it).
    const IntegralHead head = neighbour && between ? heads[i + 1] : IntegralHead{0.0f, 0u};
    const int64_t next = neighbour ? s.start_time[i + 1] : 0;
    const int64_t t_last = regular ? (d.n_total > 0 ? trend_time_at(d, d.n_total - 1) : d.start) : s.end_time[i];
    const bool link = head.rows > 0 && d.n_total > 0 && integral_linked(q.max_gap, t_last, next);
    if (closed && n_res == 0 && !link) return;
    const SampleWindow w = sample_window(r.origin, r.width, q.max_gap, q.method, k_first + (j0 - off),
                                         k_first + (j1 - off), out + (j0 - p0));
    SampleWalk walk = sample_walk_start();
    if (closed) {
        sample_walk_point(w, walk, trend_time_at(d, d.n_model - 1), d.value, false);
        if (n_res > 0) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, n_res, true, __float_as_uint(d.value), error,
                             [&](uint32_t k, uint32_t bits) {
                                 sample_walk_point(w, walk, trend_time_at(d, d.n_model + k), __uint_as_float(bits), true);
                             });
        }
    } else {
        // How far the rows are needed on regular timestamps: to the end when the link wants the last value, else one
        // row past the window's last instant.
        uint32_t limit = d.n_total;
        if (regular && !link && d.delta > 0 && d.n_total > 0) {
            if (w.t_hi < d.start) limit = 1;
            else if (w.t_hi < t_last) limit = (uint32_t)(((uint64_t)w.t_hi - (uint64_t)d.start) / (uint64_t)d.delta) + 2;
        }
        integral_rows(s, i, info, limit, error, [&](int64_t t, float v) { sample_walk_point(w, walk, t, v, true); });
    }
    if (link) sample_walk_point(w, walk, next, head.value, false);
}

} // namespace mdb

#endif // __HIPCC__
