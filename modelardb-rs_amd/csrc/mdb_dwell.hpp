// mdb_dwell.hpp - the time spent per value cell, per date_bin bucket and group (mdb_dwell_buckets*): for every LINKED
// interval (t0, v0) - (t1, v1) of the rows (mdb.h: the rule of mdb_integral_buckets) the series holds v0 on [t0, t1);
// the interval is cut at the bucket edges and each piece's microseconds are added to the cell of v0 under the edge
// list of mdb_hist_buckets. The product of mdb_integral.hpp (links, extents, the bucket walk) and mdb_hist_dev.hpp
// (the cell rule, the lane, the closed form of a Swing run).
//
// The first part is plain C++ (no HIP type): the bucket walk of one interval reduced to integers, the walk of a run of
// rows, the pieces of one bucket among rows on regular timestamps and the request's checks. It is shared by the
// kernel, by the host entry points (mdb_dwell_host.cpp) and by the check program tests/dwell_host, which runs it under
// the CPU sanitizers. The second part (hipcc only) is the lane and what it makes of one segment.
//
// Arithmetic: integers only. Every time difference is formed in uint64_t; bucket starts wrap and are exact wherever a
// real timestamp reaches them, bucket ends saturate at INT64_MAX (mdb_integral.hpp).
#pragma once

#include "mdb_hist.hpp"
#include "mdb_integral.hpp"

namespace mdb {

// The buckets [b0, b1) a walk may add to: those a real timestamp of the segment's extent reaches (the span's promise).
struct DwellWindow {
    int64_t origin, width, max_gap;
    uint64_t b0, b1;
};

// The linked interval [t0, t1), t1 > t0, over the window's buckets: emit(bucket, microseconds) per bucket it overlaps.
// integral_walk_interval without the values.
template <typename Emit>
MDB_INTEGRAL_FN void dwell_interval(const DwellWindow &w, int64_t t0, int64_t t1, Emit emit) {
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
        emit(b, (uint64_t)e - (uint64_t)a);
        if (t1 <= end) break;
        b++;
    }
}

// A run of rows of one group, fed in row order: the key of the earlier row of every linked pair is held up to the later.
struct DwellWalk {
    int64_t t_prev;
    int32_t key_prev;
    bool have;
};

MDB_INTEGRAL_FN DwellWalk dwell_walk_start() { return DwellWalk{0, 0, false}; }

// The next row of the run: emit(bucket, key, microseconds) per piece of the interval that ends at it.
template <typename Emit>
MDB_INTEGRAL_FN void dwell_walk_point(const DwellWindow &w, DwellWalk &walk, int64_t t, int32_t key, Emit emit) {
    if (walk.have && integral_linked(w.max_gap, walk.t_prev, t)) {
        const int32_t held = walk.key_prev;
        dwell_interval(w, walk.t_prev, t, [&](uint64_t b, uint64_t length) { emit(b, held, length); });
    }
    walk.have = true;
    walk.t_prev = t;
    walk.key_prev = key;
}

// The share of bucket [bucket_start, bucket_end) in the rows k in [0, n) at start + k * delta, delta > 0, every two
// neighbours linked - a model on regular timestamps. Row k holds its value on [t_k, t_k+1), row n - 1 holds nothing:
//   head   microseconds of row head_row, whose interval the bucket's start cuts (or that holds the whole bucket)
//   whole  rows [ka, kb): `delta` microseconds each
//   tail   microseconds of row kb, whose interval the bucket's end cuts
// Everything 0 when the bucket does not overlap [start, t_(n-1)).
struct DwellRegular {
    uint64_t head, tail;
    uint32_t head_row, ka, kb;
};

MDB_INTEGRAL_FN DwellRegular dwell_regular_bucket(int64_t start, int64_t delta, uint32_t n, int64_t bucket_start,
                                                  int64_t bucket_end) {
    DwellRegular p = {0, 0, 0, 0, 0};
    if (n < 2) return p;
    const int64_t last = (int64_t)((uint64_t)start + (uint64_t)(n - 1) * (uint64_t)delta);
    const int64_t a = start > bucket_start ? start : bucket_start, e = last < bucket_end ? last : bucket_end;
    if (e <= a) return p;
    const uint64_t step = (uint64_t)delta, from = (uint64_t)a - (uint64_t)start, to = (uint64_t)e - (uint64_t)start;
    const uint32_t ka = (uint32_t)(from / step + (from % step != 0)); // the first row at or behind a (<= n - 1)
    const uint32_t kb = (uint32_t)(to / step);                        // the last row at or before e
    if (kb < ka) { // (kb == ka - 1: the bucket lies inside one interval)
        p.head = (uint64_t)e - (uint64_t)a;
        p.head_row = kb;
        return p;
    }
    p.ka = ka;
    p.kb = kb;
    if (ka > 0) {
        p.head = (uint64_t)ka * step - from;
        p.head_row = ka - 1;
    }
    p.tail = to - (uint64_t)kb * step;
    return p;
}

// The host-side checks every form makes before it touches the device: those of mdb_integral_buckets* and
// mdb_hist_buckets* together; *n_rows = n_groups * n_buckets, with n_edges + 1 counters each.
inline int dwell_request_check(const mdb_dwell_request *request, uint32_t n_edges, uint64_t *n_rows) {
    const mdb_bucket_request &b = request->buckets;
    if (b.which_mask != 0) return fail("which_mask must be 0 for mdb_dwell_buckets*.");
    if (b.width <= 0) return fail("The bucket width must be positive.");
    if (b.n_groups == 0) return fail("n_groups must be at least 1.");
    if (b.t_lo != INT64_MIN || b.t_hi != INT64_MAX)
        return fail("mdb_dwell_buckets* takes no time range: t_lo / t_hi must be INT64_MIN / INT64_MAX.");
    if (request->method == MDB_INTEGRAL_LINEAR)
        return fail("Method 0 (MDB_INTEGRAL_LINEAR's number) is refused by mdb_dwell_buckets*: a line crosses an edge "
                    "between two microseconds. MDB_DWELL_STEP is the only method.");
    if (request->method != MDB_DWELL_STEP) return fail("Unknown method: MDB_DWELL_STEP is the only one.");
    if (request->flags != 0) return fail("mdb_dwell_request.flags must be 0.");
    if (request->max_gap < 0) return fail("max_gap must not be negative.");
    const unsigned __int128 rows = (unsigned __int128)b.n_groups * b.n_buckets;
    if (rows * ((uint64_t)n_edges + 1) > (unsigned __int128)(UINT64_MAX / 16))
        return fail("n_groups * n_buckets * n_cells overflows.");
    *n_rows = (uint64_t)rows;
    return 0;
}

// mdb_dwell.hip: the host batches of the list uploaded and their microseconds added to the caller's counters (the
// request and the edges checked, the list not empty). The only step of the host forms that needs the device.
int dwell_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                   uint32_t n_inputs, const mdb_dwell_request *request, const std::vector<int32_t> &edge_keys,
                   uint64_t n_rows, uint64_t *dwell);

} // namespace mdb

#if defined(__HIPCC__)

#include "mdb_hist_dev.hpp"

namespace mdb {

// The lane of the edge list, weighted by time: mdb_hist_dev.hpp's lane contract, so HistCellsOf<DwellLane>::model
// serves for a Swing run. `run` counts in units of `unit` microseconds - 1 for a piece, the sampling interval for the
// whole intervals of a run of rows - and is multiplied out when it is flushed.
struct DwellLane {
    const int32_t *edges;      // the edges' keys (LDS)
    uint32_t n_edges;
    unsigned long long *cells; // the row of the segment's group and bucket
    int32_t lo, hi;            // the keys of the current cell, closed (lo > hi: no cell yet)
    uint32_t cell;
    unsigned long long run;    // units of the current cell not added yet
    unsigned long long unit;   // microseconds per unit

    __device__ __forceinline__ uint32_t cell_of(int32_t key) const {
        uint32_t a = 0, b = n_edges;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (edges[mid] <= key) a = mid + 1;
            else b = mid;
        }
        return a;
    }
    __device__ __forceinline__ void flush() {
        if (run) atomicAdd(&cells[cell], run * unit);
        run = 0;
    }
    __device__ __forceinline__ void add(int32_t key, unsigned long long n) {
        if (key < lo || key > hi) {
            flush();
            cell = cell_of(key);
            lo = cell == 0 ? INT32_MIN : edges[cell - 1];
            hi = cell == n_edges ? INT32_MAX : edges[cell] - 1; // (edges[cell] > key: no wrap)
        }
        run += n;
    }
    // What follows is added to `row`, in units of `microseconds`.
    __device__ __forceinline__ void aim(unsigned long long *row, unsigned long long microseconds) {
        if (row != cells || microseconds != unit) {
            flush();
            cells = row;
            unit = microseconds;
        }
    }
};

// Does segment j rebuild to a row? A well-formed segment does not only under a stored length with end_time <
// start_time (analyse_segment). Judged from the views and times alone, where k_integral_heads analyses the segment: a
// malformed one fails the call in its own lane where a bucket reaches it, and is not reported where none does (mdb.h
// says so) - it then counts as a segment with rows, unless its view's length is negative.
__device__ __forceinline__ bool dwell_has_rows(const DevSegments &s, uint64_t j) {
    const int32_t ts_len = (int32_t)s.timestamps.views[j].x;
    if (ts_len <= 0) return ts_len == 0;
    return !segment_has_regular_timestamps(s, j) || s.end_time[j] >= s.start_time[j];
}

// Segment i, whose extent reaches the buckets [b_first, b_first + count), into the rows row0 + bucket of `cells`
// (row0 = group * n_buckets); the link to its right neighbour is the segment's own. PMC-Mean on regular timestamps:
// the model's rows are one constant stretch, one add per bucket. Swing on regular timestamps: per bucket the pieces
// of dwell_regular_bucket, the whole intervals through HistCellsOf::model. Then only the residual tail and the link
// are walked, behind the model's last row. Everything else - MacaqueV values, irregular timestamps, a sampling
// interval the gap rule does not link - is one walk of the rows.
__device__ __forceinline__ void dwell_segment(const DevSegments &s, const uint32_t *groups, uint64_t i, const SegInfo &info,
                                              const IntegralRequest &q, uint64_t b_first, uint64_t count, uint64_t row0,
                                              DwellLane &lane, unsigned long long *cells, uint32_t *error) {
    const SegDesc &d = info.desc;
    const BucketRequest &r = q.buckets;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const bool regular = (d.flags & FLAG_REGULAR) != 0;
    const DwellWindow w = {r.origin, r.width, q.max_gap, b_first, b_first + count};
    const uint64_t row_cells = (uint64_t)lane.n_edges + 1;
    auto key_of = [](float v) { return total_order_key(__float_as_uint(v)); };
    auto piece = [&](uint64_t b, int32_t key, uint64_t length) {
        lane.aim(cells + (row0 + b) * row_cells, 1);
        lane.add(key, length);
    };
    const bool model = regular && type != MDB_MACAQUE_V_ID && d.n_model >= 1;
    const bool closed = model && d.n_model >= 2 && integral_linked(q.max_gap, 0, d.delta);
    if (closed && type == MDB_PMC_MEAN_ID) {
        const int32_t key = key_of(d.value);
        dwell_interval(w, d.start, trend_time_at(d, d.n_model - 1), [&](uint64_t b, uint64_t length) { piece(b, key, length); });
    } else if (closed) {
        const HistCellsOf<DwellLane> sel{&lane};
        RangeAcc unused;
        for (uint64_t b = w.b0; b < w.b1; b++) {
            const int64_t start = integral_bucket_start(r.origin, r.width, b);
            const DwellRegular p = dwell_regular_bucket(d.start, d.delta, d.n_model, start, integral_bucket_end(start, r.width));
            if (p.head) piece(b, key_of(swing_value_at(d, p.head_row)), p.head);
            if (p.kb > p.ka) {
                lane.aim(cells + (row0 + b) * row_cells, (unsigned long long)d.delta);
                sel.model(d, type, p.ka, p.kb - 1, 0, unused);
            }
            if (p.tail) piece(b, key_of(swing_value_at(d, p.kb)), p.tail);
        }
    }
    // The link is walked when the rows' own rule may link it; the last row's time is arithmetic on regular timestamps
    // and end_time on irregular ones (the stream does not store it). Its far end is the neighbour's start_time: no
    // value of the neighbour is read.
    const bool neighbour = i + 1 < s.n && integral_same_group(groups, i, i + 1);
    const int64_t next = neighbour ? s.start_time[i + 1] : 0;
    const int64_t t_last = regular ? (d.n_total > 0 ? trend_time_at(d, d.n_total - 1) : d.start) : s.end_time[i];
    const bool link = neighbour && d.n_total > 0 && integral_linked(q.max_gap, t_last, next) && dwell_has_rows(s, i + 1);
    DwellWalk walk = dwell_walk_start();
    auto point = [&](int64_t t, float v) { dwell_walk_point(w, walk, t, key_of(v), piece); };
    const uint32_t n_res = d.n_total - d.n_model;
    if (model) {
        if (n_res > 0 || link) point(trend_time_at(d, d.n_model - 1), d.value);
        if (n_res > 0) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, n_res, true, __float_as_uint(d.value), error,
                             [&](uint32_t k, uint32_t bits) { point(trend_time_at(d, d.n_model + k), __uint_as_float(bits)); });
        }
    } else {
        // How far the rows are needed on regular timestamps: to the end when the link wants the last value, else one
        // row past the window's last instant.
        uint32_t limit = d.n_total;
        if (regular && !link && d.delta > 0 && d.n_total > 0) {
            const int64_t window_end = integral_bucket_end(integral_bucket_start(r.origin, r.width, w.b1 - 1), r.width);
            if (window_end <= d.start) limit = 1;
            else if (window_end <= t_last) {
                const uint64_t to = (uint64_t)window_end - (uint64_t)d.start, step = (uint64_t)d.delta;
                limit = (uint32_t)min((uint64_t)d.n_total, to / step + (to % step != 0) + 1);
            }
        }
        integral_rows(s, i, info, limit, error, point);
    }
    if (link) point(next, 0.0f);
}

} // namespace mdb

#endif // __HIPCC__
