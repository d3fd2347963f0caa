// mdb_binned.hip - the moments of one field per value cell of another, on segments (mdb_binned_buckets*): per date_bin
// bucket, group and cell of x the count, the mean and m2 of the y values of the pairs whose x value falls in the cell -
// the power curve (mean and standard deviation of active_power per cell of wind_speed), or any statistic of one field
// grouped by the value of another.
//
// What the reference answers with GridExec per field -> SortedJoinExec -> AggregateExec GROUP BY width_bucket(x, ...),
// every point of both fields rebuilt. Here the pairs, the rows and the y column are those of mdb_comoments.hip, the cell
// rule and its lane those of mdb_hist_dev.hpp, the cell and its reduction those of mdb_moments.hip. What this file adds
// is the walk that cuts an x segment into RUNS - maximal stretches of consecutive pairs inside one bucket and one cell
// of x - and reduces y over each run. Unlike a (segment, bucket) pair, the number of runs of a segment is not known
// from its bucket span, so the walk is made twice:
//
//   rows, first rows, ycol  comoments_rows (mdb_comoments.hip): the row counts of x and y compared, x's first rows, the
//                           range grid of y, values only, in scratch: 4 B per row, in HBM only.
//   k_hist_bucket_slots     (mdb_hist_buckets.hip) 8 B per (segment, bucket) of the segments whose timestamps are
//                           irregular AND whose values are a bit stream: their index interval per bucket.
//   k_binned_count          1 lane / x segment: the group id checked on every row; the runs of the segments the request
//                           reaches counted. No y is read. PMC-Mean on regular timestamps: one run per bucket reached,
//                           O(1) each. Swing on regular timestamps: per bucket the index intervals per cell from the
//                           monotone search of HistCellsOf::model. Streams of values or timestamps: decoded a constant
//                           number of times, whatever number of buckets the segment reaches (the walk is that of
//                           k_hist_buckets). A scan makes run offsets; they are read back once to cut the slices.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS runs, slices folded one after the other (a slice ends only at
//   a segment boundary: a segment with more runs than that is a slice of its own):
//   k_binned_partials       the same walk; per run {key = (group * n_buckets + bucket) * n_cells + cell, the cell of
//                           ycol[row .. row + n)} - the run summed around its first y value (mdb_moments.hpp). The row
//                           of a pair is the one the by_row selectors see: the segment's first row plus the number of
//                           its earlier points inside [t_lo, t_hi].
//   k_agg_bucket_check      (shared) keys non-decreasing? If not, a stable radix sort by key.
//   k_moments_tree / _fold  the one tree and fold of every per-bucket operator (mdb_bucket_fold.hpp), instantiated here
//                           with mdb_moments.hpp's MomentsFoldOps under the names mdb_moments.hip's launches have: runs
//                           of equal keys reduced through the fixed tree and merged into the cell. No two lanes write
//                           one cell, no atomics on cells.
// Both walks are one function with two sinks, so they cut the same runs; a segment whose second walk does not produce
// the number of runs its first walk counted fails the call (ERR_BINNED_RUNS) before anything is folded. Runs meet only
// in moments_merge, in an order fixed by the input, the request, the edges and the slice size. The batch's cursor index
// is not used (as k_hist). All stores are ordinary vector stores.
//
// Known weakness (MEASUREMENTS.md): one lane reduces one run, so the lanes of a wave read ycol a segment apart.
//
// Scratch: 4 B per row of y, 32 B per run of a slice (the cell and the key), 16 B per segment of x (counts, offsets),
// 12 B per segment for the row plan, the edges' keys.
#include "mdb_binned.hpp"
#include "mdb_comoments.hpp"
#include "mdb_hist_dev.hpp"
#include "mdb_scan.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace mdb {

constexpr uint32_t ERR_BINNED_RUNS = 1u << 29; // the two walks of a segment disagree on its runs

// The sink of k_binned_count: a run is counted.
struct RunCounter {
    unsigned long long n;
    __device__ __forceinline__ void run(uint64_t, uint32_t, uint64_t, unsigned long long) { n++; }
};

// The sink of k_binned_partials: run number n of the segment becomes entry n of the segment's `limit` entries.
struct RunWriter {
    mdb_moments_cell *out;
    unsigned long long *keys;
    uint64_t limit, n;
    uint64_t row0;    // group * n_buckets
    uint64_t n_cells; // per (group, bucket)
    YColumn y;
    uint32_t *error;
    __device__ __forceinline__ void run(uint64_t bucket, uint32_t cell, uint64_t row, unsigned long long length) {
        if (n < limit) {
            MomentsRun sums = moments_run_empty();
            for (unsigned long long k = 0; k < length; k++) moments_point(sums, y.at(row + k, error));
            out[n] = moments_finish(sums);
            keys[n] = (row0 + bucket) * n_cells + cell;
        } else {
            *error |= ERR_BINNED_RUNS;
        }
        n++;
    }
};

// A lane of HistCellsOf (mdb_hist_dev.hpp) that remembers where its run began: `run` pairs from row `row` on, all in
// bucket `bucket` and cell `cell` of x. Points arrive in row order; seek() says where the next one lies.
template <typename Sink>
struct BinnedLane {
    const int32_t *edges; // the edges' keys (LDS)
    uint32_t n_edges;
    Sink *sink;
    int32_t lo, hi; // the keys of the current cell, closed (lo > hi: no cell yet)
    uint32_t cell;
    unsigned long long run;
    uint64_t bucket, row;

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
        if (run) sink->run(bucket, cell, row, run);
        row += run;
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
    // The next point added is row `at`, in bucket b: the run goes on only if it is the next row of the same bucket.
    __device__ __forceinline__ void seek(uint64_t b, uint64_t at) {
        if (b != bucket || at != row + run) {
            flush();
            bucket = b;
            row = at;
        }
    }
};

// The values of segment i that are a bit stream, or a model under irregular timestamps in front of a residual tail:
// points [0, needed) decoded once, visit(k, v) for each (pass 2 of hist_buckets_segment).
template <typename Visit>
__device__ __forceinline__ void binned_stream_values(const DevSegments &s, uint64_t i, const SegInfo &info, uint32_t needed,
                                                     uint32_t *error, const Visit &visit) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const uint32_t n_res = d.n_total - d.n_model;
    if (needed == 0) return;
    float seed = d.value;
    if (type == MDB_MACAQUE_V_ID) {
        const uint4 vv = s.values.views[i];
        uint32_t last_bits = 0;
        const bool residuals_needed = n_res > 0 && needed > d.n_model;
        decode_macaque_v(view_data(s.values, i, vv), vv.x, residuals_needed ? d.n_model : min(d.n_model, needed), false, 0,
                         error, [&](uint32_t k, uint32_t bits) {
                             visit(k, __uint_as_float(bits));
                             last_bits = bits;
                         });
        seed = __uint_as_float(last_bits);
    } else if (d.n_model > 0) { // PMC-Mean / Swing under a residual tail: the model at each of its timestamps
        const uint4 vt = s.timestamps.views[i];
        decode_irregular_timestamps(view_data(s.timestamps, i, vt), vt.x, d.start, s.end_time[i], min(d.n_model, needed),
                                    error, [&](uint32_t k, int64_t t) {
                                        if (k < d.n_model) visit(k, model_value_at(d, type, t));
                                    });
    }
    if (n_res > 0 && needed > d.n_model) {
        const uint4 vr = s.residuals.views[i];
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, needed - d.n_model, true, __float_as_uint(seed), error,
                         [&](uint32_t k, uint32_t bits) { visit(d.n_model + k, __uint_as_float(bits)); });
    }
}

// The pairs of x segment i inside the buckets [b_first, b_first + count) of the request, in row order, cut into runs
// by the lane: the walk of hist_buckets_segment (mdb_hist_buckets.hip) with every point's row told to the lane.
// first_row: the row of the segment's first point inside [t_lo, t_hi]. slots: the segment's `count` slots, or nullptr.
template <typename Sink>
__device__ __forceinline__ void binned_segment(const DevSegments &s, uint64_t i, const SegInfo &info, const BucketRequest &r,
                                               uint64_t b_first, uint64_t count, uint64_t first_row,
                                               BinnedLane<Sink> &lane, uint2 *slots, uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const uint32_t n_res = d.n_total - d.n_model;
    const int64_t end = s.end_time[i];
    const HistCellsOf<BinnedLane<Sink>> sel{&lane};
    RangeAcc unused;
    auto key_of = [](float v) { return total_order_key(__float_as_uint(v)); };
    // The points any bucket of the request holds: [clip_lo, clip_hi].
    const int64_t clip_lo = r.t_lo > r.origin ? r.t_lo : r.origin;
    const int64_t last_time = buckets_last_time(r);
    const int64_t clip_hi = r.t_hi < last_time ? r.t_hi : last_time;
    if (clip_lo > clip_hi) return;

    if (d.flags & FLAG_REGULAR) {
        uint32_t k_first = 0, k_range_last = 0; // the segment's points inside [t_lo, t_hi]: point k_first is its row 0
        (void)regular_index_interval(d.start, d.delta, d.n_total, r.t_lo, r.t_hi, &k_first, &k_range_last);
        const uint64_t row_base = first_row - k_first; // (wrapping: row_base + k is exact for every k >= k_first)
        // The model's points: per bucket its index interval, cut by cell in closed form.
        if (type != MDB_MACAQUE_V_ID && d.n_model > 0) {
            for (uint64_t b = b_first; b < b_first + count; b++) {
                int64_t lo, hi;
                bucket_bounds(r, b, &lo, &hi);
                uint32_t k_lo = 0, k_hi = 0;
                if (!regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi) || k_lo >= d.n_model) continue;
                lane.seek(b, row_base + k_lo);
                sel.model(d, type, k_lo, min(k_hi, d.n_model - 1), 0, unused);
            }
        }
        if (type != MDB_MACAQUE_V_ID && n_res == 0) return;
        // The bit streams: decoded once; the bucket of point k is arithmetic, a division where the bucket changes.
        uint32_t k_lo = 0, k_hi = 0;
        if (!regular_index_interval(d.start, d.delta, d.n_total, clip_lo, clip_hi, &k_lo, &k_hi)) return;
        uint32_t k_last = 0; // the last index of the current bucket
        bool placed = false; // k_last is valid, and the bucket is one of the segment's
        uint64_t bucket = 0;
        auto visit = [&](uint32_t k, float v) {
            if (k < k_lo || k > k_hi) return;
            if (!placed || k > k_last) {
                const int64_t t = d.start + (int64_t)((uint64_t)k * (uint64_t)d.delta);
                const uint64_t b = ((uint64_t)t - (uint64_t)r.origin) / (uint64_t)r.width; // (t >= origin: inside the clip)
                placed = b >= b_first && b - b_first < count;
                k_last = k;
                if (!placed) return;
                if (d.delta > 0) {
                    int64_t lo, hi;
                    bucket_bounds(r, b, &lo, &hi);
                    const uint64_t reach = ((uint64_t)hi - (uint64_t)d.start) / (uint64_t)d.delta;
                    k_last = reach < k_hi ? (uint32_t)reach : k_hi;
                }
                bucket = b;
            }
            lane.seek(bucket, row_base + k);
            lane.add(key_of(v), 1);
        };
        float seed = d.value;
        if (type == MDB_MACAQUE_V_ID) {
            const uint4 vv = s.values.views[i];
            uint32_t last_bits = 0;
            const bool residuals_in_range = n_res > 0 && k_hi >= d.n_model;
            const uint32_t upto = residuals_in_range ? d.n_model : min(d.n_model, k_hi + 1);
            if (k_lo < d.n_model || residuals_in_range)
                decode_macaque_v(view_data(s.values, i, vv), vv.x, upto, false, 0, error, [&](uint32_t k, uint32_t bits) {
                    visit(k, __uint_as_float(bits));
                    last_bits = bits;
                });
            seed = __uint_as_float(last_bits);
        }
        if (n_res > 0 && k_hi >= d.n_model) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, k_hi - d.n_model + 1, true, __float_as_uint(seed),
                             error, [&](uint32_t k, uint32_t bits) { visit(d.n_model + k, __uint_as_float(bits)); });
        }
        return;
    }

    // Irregular timestamps.
    const uint4 vt = s.timestamps.views[i];
    const uint8_t *ts_bytes = view_data(s.timestamps, i, vt);
    // The bucket of timestamp t among the segment's, as a slot number; false: the request does not hold the point.
    auto slot_of = [&](int64_t t, uint64_t *slot) {
        if (t < clip_lo || t > clip_hi) return false;
        const uint64_t b = ((uint64_t)t - (uint64_t)r.origin) / (uint64_t)r.width;
        if (b < b_first || b - b_first >= count) return false;
        *slot = b - b_first;
        return true;
    };
    if (type != MDB_MACAQUE_V_ID && n_res == 0) {
        // The model at every timestamp: one decode, every point placed by its own timestamp (sorted or not), its row
        // the running count of the points inside [t_lo, t_hi] (what segment_range calls the row).
        int64_t lo = 1, hi = 0;
        uint64_t row = first_row, bucket = 0;
        decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t, int64_t t) {
            if (t < r.t_lo || t > r.t_hi) return;
            const uint64_t at = row;
            row += 1;
            if (t < lo || t > hi) {
                uint64_t slot;
                if (!slot_of(t, &slot)) return;
                bucket_bounds(r, b_first + slot, &lo, &hi);
                bucket = b_first + slot;
            }
            lane.seek(bucket, at);
            lane.add(key_of(model_value_at(d, type, t)), 1);
        });
        return;
    }
    // Values in a bit stream. Pass 1: the index interval [x, y] of every reached bucket (x > y: none) into the slots,
    // and the index of the first point inside [t_lo, t_hi] (row 0 of the segment).
    if (!slots) { // (k_hist_bucket_slots gives every such segment its slots: not reached)
        *error |= ERR_TIMESTAMPS;
        return;
    }
    for (uint64_t j = 0; j < count; j++) slots[j] = make_uint2(1, 0);
    uint64_t open = ~0ull;
    uint32_t x = 0, y = 0, k_first = 0;
    int64_t previous = INT64_MIN;
    bool sorted = true, any_in_range = false;
    decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t k, int64_t t) {
        if (t < previous) sorted = false;
        previous = t;
        if (!sorted || t < r.t_lo || t > r.t_hi) return;
        if (!any_in_range) {
            any_in_range = true;
            k_first = k;
        }
        uint64_t slot;
        if (!slot_of(t, &slot)) return;
        if (slot != open) {
            if (open != ~0ull) slots[open] = make_uint2(x, y);
            open = slot;
            x = k;
        }
        y = k;
    });
    if (!sorted) {
        // A malformed stream: bucket by bucket, the points comoments_unsorted_pair (and the range aggregate) takes for
        // the bucket's bounds - the indices between the first and the last timestamp inside them, point k at row
        // k - the first index inside [t_lo, t_hi].
        for (uint64_t b = b_first; b < b_first + count; b++) {
            int64_t lo, hi;
            bucket_bounds(r, b, &lo, &hi);
            if (end < lo || d.start > hi) continue;
            uint32_t k_lo = 0xffffffffu, k_hi = 0, k_row0 = 0xffffffffu;
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t k, int64_t t) {
                if (t >= r.t_lo && t <= r.t_hi && k < k_row0) k_row0 = k;
                if (t >= lo && t <= hi) {
                    if (k < k_lo) k_lo = k;
                    if (k > k_hi) k_hi = k;
                }
            });
            if (k_lo == 0xffffffffu) continue;
            binned_stream_values(s, i, info, k_hi + 1, error, [&](uint32_t k, float v) {
                if (k < k_lo || k > k_hi) return;
                lane.seek(b, first_row + (k - k_row0));
                lane.add(key_of(v), 1);
            });
        }
        return;
    }
    if (open == ~0ull) return;
    slots[open] = make_uint2(x, y);
    // Pass 2: the values decoded once, up to point y; the intervals are ascending and disjoint.
    uint64_t j = 0;
    uint2 current = slots[0];
    const uint64_t row_base = first_row - k_first;
    binned_stream_values(s, i, info, y + 1, error, [&](uint32_t k, float v) {
        while (j < count && (current.x > current.y || k > current.y)) {
            j++;
            if (j < count) current = slots[j];
        }
        if (j == count || k < current.x) return;
        lane.seek(b_first + j, row_base + k);
        lane.add(key_of(v), 1);
    });
}

// The edges' keys into LDS (every thread of the workgroup calls this).
__device__ __forceinline__ void binned_load_edges(int32_t *lds, const int32_t *__restrict__ edge_keys, uint32_t n_edges) {
    for (uint32_t j = threadIdx.x; j < n_edges; j += BUCKET_THREADS) lds[j] = edge_keys[j];
    __syncthreads();
}

__device__ __forceinline__ uint2 *binned_slots_of(const DevSegments &s, uint64_t i, uint64_t count,
                                                  const unsigned long long *slot_offsets, uint2 *slots) {
    if (slots && hist_bucket_wants_slots(s, i) && slot_offsets[i + 1] - slot_offsets[i] == count) return slots + slot_offsets[i];
    return nullptr;
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_binned_count(
    DevSegments s, const uint32_t *__restrict__ groups, BucketRequest r, const int32_t *__restrict__ edge_keys,
    uint32_t n_edges, const unsigned long long *__restrict__ slot_offsets, uint2 *__restrict__ slots,
    const unsigned long long *__restrict__ first_row, unsigned long long *__restrict__ counts,
    unsigned int *__restrict__ error_out) {
    __shared__ int32_t lds_keys[MDB_HIST_MAX_EDGES + 1];
    binned_load_edges(lds_keys, edge_keys, n_edges);
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= s.n) return;
    uint32_t error = 0;
    unsigned long long runs = 0;
    uint64_t b_first = 0;
    const uint64_t count = bucket_span(s.start_time[i], s.end_time[i], r, &b_first);
    if (groups && groups[i] >= r.n_groups) {
        error = ERR_BUCKET_GROUP; // (on every row, also one the request does not reach)
    } else if (count > 0) {
        const SegInfo info = analyse_segment(s, i);
        error = info.error;
        if (!error) {
            RunCounter sink{0};
            BinnedLane<RunCounter> lane{lds_keys, n_edges, &sink, 1, 0, 0, 0, 0, 0};
            binned_segment(s, i, info, r, b_first, count, first_row[i], lane, binned_slots_of(s, i, count, slot_offsets, slots),
                           &error);
            lane.flush();
            runs = sink.n;
        }
    }
    counts[i] = error ? 0 : runs;
    if (error) atomicOr(error_out, error);
}

// Segments [i0, i1) of the batch, whose runs are entries [e0, offsets[i1]) of the call: entry e at e - e0.
__global__ __launch_bounds__(BUCKET_THREADS) void k_binned_partials(
    DevSegments s, const uint32_t *__restrict__ groups, BucketRequest r, const int32_t *__restrict__ edge_keys,
    uint32_t n_edges, const unsigned long long *__restrict__ slot_offsets, uint2 *__restrict__ slots,
    const unsigned long long *__restrict__ first_row, YColumn y, const unsigned long long *__restrict__ offsets,
    uint64_t i0, uint64_t i1, uint64_t e0, mdb_moments_cell *__restrict__ out, unsigned long long *__restrict__ keys,
    unsigned int *__restrict__ error_out) {
    __shared__ int32_t lds_keys[MDB_HIST_MAX_EDGES + 1];
    binned_load_edges(lds_keys, edge_keys, n_edges);
    const uint64_t i = i0 + (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= i1) return;
    const uint64_t off = offsets[i], stop = offsets[i + 1];
    if (off >= stop || off < e0) return;
    uint64_t b_first = 0;
    const uint64_t count = bucket_span(s.start_time[i], s.end_time[i], r, &b_first);
    const SegInfo info = analyse_segment(s, i);
    uint32_t error = info.error;
    RunWriter sink{out + (off - e0), keys + (off - e0), stop - off, 0, (uint64_t)(groups ? groups[i] : 0u) * r.n_buckets,
                   (uint64_t)n_edges + 1, y, &error};
    if (!error && count > 0) {
        BinnedLane<RunWriter> lane{lds_keys, n_edges, &sink, 1, 0, 0, 0, 0, 0};
        binned_segment(s, i, info, r, b_first, count, first_row[i], lane, binned_slots_of(s, i, count, slot_offsets, slots),
                       &error);
        lane.flush();
    }
    if (sink.n != sink.limit) error |= ERR_BINNED_RUNS;
    if (error) atomicOr(error_out, error);
}

static int binned_error(unsigned int error) {
    if (error & ERR_BUCKET_GROUP) return fail("A group id is not below n_groups.");
    if (error & ERR_COMOMENTS_ROW)
        return fail("(internal) A row of the x field lies beyond the y column: the row plan and the range grid disagree.");
    if (error & ERR_BINNED_RUNS) return fail("(internal) The two walks of an x segment disagree on its runs.");
    if (error) return fail(describe_error(error));
    return 0;
}

// The pairs of the device batches x and y (groups: a device array or nullptr) merged into a device array of n_cells
// cells. `host_cells` (host forms): the caller's array, which is uploaded, merged into and downloaded instead; either
// way nothing of the caller's is written unless the whole call succeeds.
static int binned_run(mdb_ctx *ctx, const mdb_segments *in, const mdb_segments *y_in, const uint32_t *groups,
                      const mdb_bucket_request *request, const std::vector<int32_t> &edge_keys, uint64_t n_cells,
                      mdb_moments_cell *dev_cells, mdb_moments_cell *host_cells) {
    const uint64_t n = in->n;
    if (n == 0 || request->n_buckets == 0) return 0;
    const BucketRequest r = {request->origin, request->width, request->n_buckets, request->t_lo, request->t_hi,
                             request->n_groups, request->which_mask};
    const uint32_t n_edges = (uint32_t)edge_keys.size();
    if (hist_buckets_fits(n_cells * sizeof(mdb_moments_cell), "n_groups * n_buckets * n_cells cells")) return 1;
    const unsigned long long *first_row = nullptr;
    YColumn y{nullptr, 0};
    if (comoments_rows(ctx, in, y_in, r.t_lo, r.t_hi, &first_row, &y)) return 1;
    const DevSegments s = to_dev(in);
    HistSlots slots;
    if (hist_buckets_slots(ctx, in, s, r, &slots)) return 1;

    void *p = nullptr;
    const uint64_t per_segment = align_up((n + 1) * 8, 256);
    if (scratch_reserve(ctx, SCRATCH_BINNED, 2 * per_segment + align_up(scan_block_sums_bytes(n), 256) +
                                                 align_up((uint64_t)n_edges * 4, 256) + 256, &p))
        return 1;
    Carver scratch(p);
    unsigned long long *counts = scratch.take<unsigned long long>(n + 1);
    unsigned long long *offsets = scratch.take<unsigned long long>(n + 1);
    unsigned long long *block_sums = scratch.take<unsigned long long>(scan_block_sums_bytes(n) / 8);
    int32_t *keys_dev = scratch.take<int32_t>(n_edges);
    unsigned int *words = scratch.take<unsigned int>(2);
    MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
    MDB_HIP_CHECK(mail_write(ctx, keys_dev, edge_keys.data(), (uint64_t)n_edges * 4));
    {
        LaunchTimer timer(ctx, "k_binned_count");
        hipLaunchKernelGGL(k_binned_count, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, r, keys_dev,
                           n_edges, slots.offsets, slots.slots, first_row, counts, words);
    }
    if (device_exclusive_scan(ctx, ItemsOf<unsigned long long>{counts}, n, offsets, block_sums, "k_binned_scan")) return 1;
    std::vector<unsigned long long> run_offsets(n + 1);
    unsigned int count_error = 0;
    MDB_HIP_CHECK(hipMemcpyAsync(run_offsets.data(), offsets, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipMemcpyAsync(&count_error, words, 4, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (binned_error(count_error)) return 1;
    const unsigned long long total = run_offsets[n];
    if (total == 0) return 0;

    // The slices: segments [cuts[k], cuts[k + 1]), as many as hold at most `slice` runs - at least one segment.
    const uint64_t slice = slice_pairs_setting();
    std::vector<uint64_t> cuts(1, 0);
    uint64_t cap = 0;
    while (cuts.back() < n) {
        const uint64_t i0 = cuts.back();
        uint64_t i1 = (uint64_t)(std::upper_bound(run_offsets.begin() + i0, run_offsets.end(), run_offsets[i0] + slice) -
                                 run_offsets.begin()) - 1;
        if (i1 <= i0) i1 = i0 + 1;
        cap = std::max<uint64_t>(cap, run_offsets[i1] - run_offsets[i0]);
        cuts.push_back(i1);
    }
    if (cap > BUCKET_SLICE_MAX)
        return fail("A single segment of the x field has " + std::to_string(cap) + " runs, more than one slice can hold (" +
                    std::to_string(BUCKET_SLICE_MAX) + "): use fewer edges or cut the time range.");
    const uint64_t n_slices = cuts.size() - 1;
    BucketCells<mdb_moments_cell> cells;
    if (cells.stage(ctx, n_cells, dev_cells, host_cells, n_slices)) return 1;
    BucketFold<MomentsFoldOps> fold;
    if (fold.reserve(ctx, cap, n_cells)) return 1;
    mdb_moments_cell *partials = fold.partials();
    unsigned long long *keys = fold.keys();

    for (uint64_t k = 0; k < n_slices; k++) {
        const uint64_t i0 = cuts[k], i1 = cuts[k + 1];
        const uint64_t e0 = run_offsets[i0], m = run_offsets[i1] - e0;
        if (m == 0) continue;
        MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
        {
            LaunchTimer timer(ctx, "k_binned_partials");
            hipLaunchKernelGGL(k_binned_partials, dim3(blocks_for(i1 - i0)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, r,
                               keys_dev, n_edges, slots.offsets, slots.slots, first_row, y, offsets, i0, i1, e0, partials,
                               keys, words);
        }
        unsigned int error = 0;
        bool unsorted = false;
        if (bucket_slice_check(ctx, keys, m, words, &error, &unsorted)) return 1;
        if (binned_error(error)) return 1;
        if (fold.fold_slice(ctx, m, unsorted, cells.cells())) return 1;
    }
    return cells.commit();
}

int binned_list_run(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys, uint32_t n_y,
                    const uint32_t *const *group_of_segment_x, const mdb_bucket_request *request,
                    const std::vector<int32_t> &edge_keys, uint64_t n_cells, mdb_moments_cell *inout) {
    // (uploads the library holds, as mdb_comoments_buckets_list: two batches are alive at once)
    UploadedSegments lists(ctx);
    if (lists.upload_pair(xs, n_x, ys, n_y, group_of_segment_x)) return 1;
    return binned_run(ctx, lists.segments(), lists.y_segments(), lists.groups(), request, edge_keys, n_cells, nullptr,
                      inout);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_binned_buckets_dev(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y,
                                      const uint32_t *group_of_segment_x, const mdb_bucket_request *request,
                                      const float *edges, uint32_t n_edges, mdb_moments_cell *inout) {
    if (!ctx || !x || !y || !request || !edges || !inout)
        return fail("ctx, x, y, request, edges and inout must not be NULL.");
    std::vector<int32_t> edge_keys;
    uint64_t n_cells = 0;
    if (binned_arguments_check(request, edges, n_edges, &edge_keys, &n_cells)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return binned_run(ctx, x, y, group_of_segment_x, request, edge_keys, n_cells, inout, nullptr);
}
