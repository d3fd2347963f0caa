// mdb_hist_buckets.hip - value histograms and exact quantiles per date_bin bucket and group, computed on segments
// (mdb_hist_buckets*, mdb_quantile_buckets*): counts[group][bucket][cell] in one pass over the batch, and the order
// statistics of every (group, bucket) cell in MDB_QUANTILE_BUCKETS_PASSES passes, whatever the number of cells.
//
// What the reference answers with GridExec -> AggregateExec(approx_percentile_cont / median / a histogram) GROUP BY the
// date_bin: its model-based rule (optimizer/model_simple_aggregates.rs) rewrites only COUNT / MIN / MAX / SUM / AVG, so
// every point is rebuilt first. Before this file the per-bucket form of mdb_hist_batch / mdb_quantile_batch was one call,
// and for a quantile three passes, per bucket.
//
//   k_hist_groups       (mdb_hist.hip) every row's group id checked, also the rows the request leaves out.
//   k_hist_bucket_slots 1 lane / segment: how many 8-byte slots the segment needs - one per bucket it reaches if its
//                       timestamps are irregular AND its values are a bit stream (a MacaqueV model or a residual tail),
//                       none otherwise; a scan makes offsets.
//   k_hist_buckets      1 lane / segment the request reaches, grid-strided and launched like k_hist, the lane and the
//                       selector those of k_hist (mdb_hist_dev.hpp). The lane's row is switched, and its run flushed,
//                       to (group * n_buckets + bucket) wherever the bucket changes:
//                         model on regular timestamps: per bucket the segment reaches (bucket_span / bucket_bounds /
//                           regular_index_interval) the closed form of HistCellsOf::model over that bucket's index
//                           interval - PMC-Mean one add(key, n) in O(1), Swing binary searches with swing_first_past;
//                         bit streams on regular timestamps (MacaqueV values, residual tails): decoded ONCE, the bucket
//                           of point k being arithmetic; a division only where the bucket changes;
//                         a model without residuals on irregular timestamps: the timestamps decoded once, every point
//                           placed by its own timestamp (sorted or not: what segment_range counts bucket by bucket);
//                         bit-stream values on irregular timestamps: one pass over the timestamps leaves each reached
//                           bucket's index interval in the segment's slots (8 B per (segment, bucket) of such segments
//                           only), one pass decodes the values into them. Each stream is decoded once per pass, the
//                           timestamps once more by analyse_segment. Only where the timestamps turn out not to be
//                           sorted (a malformed stream) the lane goes bucket by bucket through segment_range, which
//                           takes the points moments_unsorted_pair takes.
//                       Two instances: edges in LDS (HistLane, the histogram) and windows (WindowLane, the quantiles).
//   k_quantile_select   1 lane / (cell, rank): the selection step of mdb_select.hpp on the windows a pass has counted -
//                       the digit is appended to the rank's prefix and the remaining rank updated, on the device.
//   k_hist_fold         (mdb_hist.hip) the scratch cells added into the caller's (the _dev form).
// Integers only, integer atomics on zeroed scratch: the forms and any two runs agree bit for bit. The batch's cursor
// index is not used (as k_hist).
#include "mdb_hist.hpp"

#include "mdb_hist_dev.hpp"
#include "mdb_scan.hpp"

#include <vector>

namespace mdb {

static_assert(SELECT_PASSES == MDB_QUANTILE_BUCKETS_PASSES, "mdb.h states the passes of the selection");

// The two cell rules of k_hist_buckets: what the kernel is given, and the lane it makes of it.
struct EdgeRule {
    using Lane = HistLane;
    static constexpr uint32_t LDS_KEYS = MDB_HIST_MAX_EDGES + 1;
    const int32_t *edge_keys;
    uint32_t n_edges;
    __device__ __forceinline__ uint64_t row_cells() const { return (uint64_t)n_edges + 1; }
    __device__ __forceinline__ Lane lane(int32_t *lds, unsigned long long *cells) const {
        for (uint32_t j = threadIdx.x; j < n_edges; j += HIST_THREADS) lds[j] = edge_keys[j];
        __syncthreads();
        return Lane{lds, n_edges, cells, 1, 0, 0, 0};
    }
    __device__ __forceinline__ void row(Lane &l, unsigned long long *cells, uint64_t row) const {
        unsigned long long *to = cells + row * row_cells();
        if (to != l.cells) {
            l.flush();
            l.cells = to;
        }
    }
};
struct WindowRule {
    using Lane = WindowLane;
    static constexpr uint32_t LDS_KEYS = 1;
    const uint32_t *prefixes; // [rows][n_ranks], or nullptr in pass 0
    uint32_t n_ranks;
    uint32_t shift;
    __device__ __forceinline__ uint64_t row_cells() const { return (uint64_t)n_ranks * SELECT_DIGITS; }
    __device__ __forceinline__ Lane lane(int32_t *, unsigned long long *cells) const {
        return Lane{prefixes, n_ranks, shift, cells, 1, 0, 0, 0};
    }
    __device__ __forceinline__ void row(Lane &l, unsigned long long *cells, uint64_t row) const {
        unsigned long long *to = cells + row * row_cells();
        if (to != l.cells) {
            l.flush();
            l.cells = to;
            l.prefixes = prefixes ? prefixes + row * n_ranks : nullptr;
        }
    }
};

// The points of segment i inside the buckets [b_first, b_first + count) of the request, counted into the rows
// row0 + bucket of `cells` (row0 = group * n_buckets). slots: the segment's `count` slots, or nullptr.
template <typename Rule>
__device__ __forceinline__ void hist_buckets_segment(const DevSegments &s, uint64_t i, const SegInfo &info,
                                                     const BucketRequest &r, uint64_t b_first, uint64_t count,
                                                     uint64_t row0, const Rule &rule, typename Rule::Lane &lane,
                                                     unsigned long long *cells, uint2 *slots, uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const uint32_t n_res = d.n_total - d.n_model;
    const int64_t end = s.end_time[i];
    const HistCellsOf<typename Rule::Lane> sel{&lane};
    RangeAcc unused;
    auto key_of = [](float v) { return total_order_key(__float_as_uint(v)); };
    // The points any bucket of the request holds: [clip_lo, clip_hi].
    const int64_t clip_lo = r.t_lo > r.origin ? r.t_lo : r.origin;
    const int64_t last_time = buckets_last_time(r);
    const int64_t clip_hi = r.t_hi < last_time ? r.t_hi : last_time;
    if (clip_lo > clip_hi) return;

    if (d.flags & FLAG_REGULAR) {
        // The model's points: per bucket its index interval, in closed form.
        if (type != MDB_MACAQUE_V_ID && d.n_model > 0) {
            for (uint64_t b = b_first; b < b_first + count; b++) {
                int64_t lo, hi;
                bucket_bounds(r, b, &lo, &hi);
                uint32_t k_lo = 0, k_hi = 0;
                if (!regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi) || k_lo >= d.n_model) continue;
                rule.row(lane, cells, row0 + b);
                sel.model(d, type, k_lo, min(k_hi, d.n_model - 1), 0, unused);
            }
        }
        if (type != MDB_MACAQUE_V_ID && n_res == 0) return;
        // The bit streams: decoded once. Point k lies at start + k * delta, so its bucket is arithmetic: a division
        // where the bucket changes, a comparison of indices elsewhere.
        uint32_t k_lo = 0, k_hi = 0;
        if (!regular_index_interval(d.start, d.delta, d.n_total, clip_lo, clip_hi, &k_lo, &k_hi)) return;
        uint32_t k_last = 0; // the last index of the current bucket
        bool placed = false; // k_last is valid, and the bucket is one of the segment's
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
                rule.row(lane, cells, row0 + b);
            } else if (!placed) {
                return;
            }
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
        // The model at every timestamp: one decode, every point placed by its own timestamp; the bounds of the current
        // bucket save the division while the points stay inside it.
        int64_t lo = 1, hi = 0;
        decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t, int64_t t) {
            if (t < lo || t > hi) {
                uint64_t slot;
                if (!slot_of(t, &slot)) return;
                bucket_bounds(r, b_first + slot, &lo, &hi);
                rule.row(lane, cells, row0 + b_first + slot);
            }
            lane.add(key_of(model_value_at(d, type, t)), 1);
        });
        return;
    }
    // Values in a bit stream. Pass 1: the index interval [x, y] of every reached bucket (x > y: none) into the slots.
    if (!slots) { // (k_hist_bucket_slots gives every such segment its slots: not reached)
        *error |= ERR_TIMESTAMPS;
        return;
    }
    for (uint64_t j = 0; j < count; j++) slots[j] = make_uint2(1, 0);
    uint64_t open = ~0ull;
    uint32_t x = 0, y = 0, needed = 0;
    int64_t previous = INT64_MIN;
    bool sorted = true;
    decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t k, int64_t t) {
        if (t < previous) sorted = false;
        previous = t;
        uint64_t slot;
        if (!sorted || !slot_of(t, &slot)) return;
        if (slot != open) {
            if (open != ~0ull) slots[open] = make_uint2(x, y);
            open = slot;
            x = k;
        }
        y = k;
    });
    if (!sorted) { // a malformed stream: bucket by bucket, the points the range aggregate takes for the bucket's bounds
        for (uint64_t b = b_first; b < b_first + count; b++) {
            int64_t lo, hi;
            bucket_bounds(r, b, &lo, &hi);
            rule.row(lane, cells, row0 + b);
            segment_range(s, i, info, lo, hi, unused, error, false, sel);
        }
        return;
    }
    if (open == ~0ull) return;
    slots[open] = make_uint2(x, y);
    needed = y + 1;
    // Pass 2: the values decoded once, up to point needed - 1; the intervals are ascending and disjoint.
    uint64_t j = 0;
    uint2 current = slots[0];
    auto visit = [&](uint32_t k, float v) {
        while (j < count && (current.x > current.y || k > current.y)) {
            j++;
            if (j < count) current = slots[j];
        }
        if (j == count || k < current.x) return;
        rule.row(lane, cells, row0 + b_first + j);
        lane.add(key_of(v), 1);
    };
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
        decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, min(d.n_model, needed), error, [&](uint32_t k, int64_t t) {
            if (k < d.n_model) visit(k, model_value_at(d, type, t));
        });
    }
    if (n_res > 0 && needed > d.n_model) {
        const uint4 vr = s.residuals.views[i];
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, needed - d.n_model, true, __float_as_uint(seed), error,
                         [&](uint32_t k, uint32_t bits) { visit(d.n_model + k, __uint_as_float(bits)); });
    }
}

// cells: n_groups * n_buckets rows of rule.row_cells() zeroed counters. (A row with a bad group id is skipped here as
// well: nothing is ever added outside the cells, whatever k_hist_groups has found.)
template <typename Rule>
__global__ __launch_bounds__(HIST_THREADS) void k_hist_buckets(DevSegments s, const uint32_t *__restrict__ groups,
                                                               BucketRequest r, Rule rule,
                                                               unsigned long long *__restrict__ cells,
                                                               const unsigned long long *__restrict__ slot_offsets,
                                                               uint2 *__restrict__ slots,
                                                               unsigned int *__restrict__ error_word) {
    __shared__ int32_t lds_keys[Rule::LDS_KEYS];
    typename Rule::Lane lane = rule.lane(lds_keys, cells);
    uint32_t errors = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * HIST_THREADS + threadIdx.x; i < s.n; i += (uint64_t)gridDim.x * HIST_THREADS) {
        uint64_t b_first = 0;
        const uint64_t count = bucket_span(s.start_time[i], s.end_time[i], r, &b_first);
        if (count == 0) continue;
        const uint32_t group = groups ? groups[i] : 0u;
        if (group >= r.n_groups) {
            errors |= ERR_HIST_GROUP;
            continue;
        }
        const SegInfo info = analyse_segment(s, i);
        uint32_t error = info.error;
        if (!error) {
            uint2 *mine = nullptr;
            if (slots && hist_bucket_wants_slots(s, i) && slot_offsets[i + 1] - slot_offsets[i] == count)
                mine = slots + slot_offsets[i];
            hist_buckets_segment(s, i, info, r, b_first, count, (uint64_t)group * r.n_buckets, rule, lane, cells, mine, &error);
        }
        errors |= error;
    }
    lane.flush();
    if (errors) atomicOr(error_word, errors);
}

struct SelectQ {
    double q[MDB_QUANTILE_BUCKETS_MAX_Q];
};

// After pass `pass` has counted: lane (cell, rank) takes the digit of its rank from its window. Pass 0 has one window
// per cell, shared by the ranks: its sum is the cell's N, from which the ranks follow (rank 2 i is the floor rank of
// q[i], rank 2 i + 1 the ceil rank). A cell without a point keeps prefix 0 and is not written by the host.
__global__ __launch_bounds__(HIST_THREADS) void k_quantile_select(const unsigned long long *__restrict__ windows,
                                                                  uint64_t n_rows, uint32_t n_ranks, uint32_t pass,
                                                                  SelectQ q, unsigned long long *__restrict__ n_points,
                                                                  unsigned long long *__restrict__ remaining,
                                                                  uint32_t *__restrict__ prefixes) {
    const uint64_t lane = (uint64_t)blockIdx.x * HIST_THREADS + threadIdx.x;
    if (lane >= n_rows * n_ranks) return;
    const uint64_t row = lane / n_ranks;
    const uint32_t rank = (uint32_t)(lane % n_ranks);
    const unsigned long long *window = windows + (pass == 0 ? row : lane) * SELECT_DIGITS;
    uint64_t wanted;
    if (pass == 0) {
        uint64_t n = 0;
        for (uint32_t digit = 0; digit < SELECT_DIGITS; digit++) n += window[digit];
        if (rank == 0) n_points[row] = n;
        prefixes[lane] = 0;
        remaining[lane] = 0;
        if (n == 0) return;
        uint64_t rank_lo, rank_hi;
        select_ranks(q.q[rank / 2], n, &rank_lo, &rank_hi);
        wanted = rank % 2 ? rank_hi : rank_lo;
    } else {
        if (n_points[row] == 0) return;
        wanted = remaining[lane];
    }
    uint64_t left = 0;
    const uint32_t digit = select_digit(reinterpret_cast<const uint64_t *>(window), SELECT_DIGITS, wanted, &left);
    prefixes[lane] = (prefixes[lane] << SELECT_DIGIT_BITS) | digit;
    remaining[lane] = left;
}

// Counters (and slots) that cannot fit the device are an error, asked only where it could matter.
int hist_buckets_fits(uint64_t bytes, const char *what) {
    if (bytes <= (1ull << 30)) return 0;
    size_t free_bytes = 0, device_bytes = 0;
    MDB_HIP_CHECK(hipMemGetInfo(&free_bytes, &device_bytes));
    if (bytes > (uint64_t)device_bytes)
        return fail(std::string(what) + " (" + std::to_string(bytes) + " bytes) do not fit into the device's memory.");
    return 0;
}

// k_hist_bucket_slots' scan and the slots themselves (SCRATCH_HIST_BUCKET_SLOTS).
int hist_buckets_slots(mdb_ctx *ctx, const mdb_segments *in, const DevSegments &s, const BucketRequest &r, HistSlots *out) {
    const uint64_t n = in->n;
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_HIST_BUCKET_OFFSETS, (n + 1) * 8 + scan_block_sums_bytes(n) + 256, &p)) return 1;
    Carver scratch(p);
    unsigned long long *offsets = scratch.take<unsigned long long>(n + 1);
    unsigned long long *block_sums = scratch.take<unsigned long long>(scan_block_sums_bytes(n) / 8);
    if (device_exclusive_scan(ctx, HistSlotCount{s, r}, n, offsets, block_sums, "k_hist_bucket_slots")) return 1;
    unsigned long long total = 0;
    MDB_HIP_CHECK(hipMemcpyAsync(&total, offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    out->offsets = offsets;
    out->slots = nullptr;
    if (total == 0) return 0;
    if (total > UINT64_MAX / 16) return fail("Too many (segment, bucket) pairs for one call: split the batch.");
    if (hist_buckets_fits(total * 8, "The index intervals of the segments with irregular timestamps")) return 1;
    if (scratch_reserve(ctx, SCRATCH_HIST_BUCKET_SLOTS, total * 8, &p)) return 1;
    out->slots = static_cast<uint2 *>(p);
    return 0;
}

namespace {

// The checks on a request every form makes before it touches the device: those of mdb_m4_buckets*; *n_rows =
// n_groups * n_buckets, with row_cells counters each.
int hist_buckets_request_check(const mdb_bucket_request *request, uint64_t row_cells, const char *what, uint64_t *n_rows) {
    if (request->which_mask != 0) return fail(std::string("which_mask must be 0 for ") + what + ".");
    if (request->width <= 0) return fail("The bucket width must be positive.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    const unsigned __int128 rows = (unsigned __int128)request->n_groups * request->n_buckets;
    if (rows * row_cells > (unsigned __int128)(UINT64_MAX / 16)) return fail("n_groups * n_buckets * n_cells overflows.");
    *n_rows = (uint64_t)rows;
    return 0;
}

BucketRequest bucket_request_of(const mdb_bucket_request *request) {
    return BucketRequest{request->origin, request->width, request->n_buckets, request->t_lo, request->t_hi,
                         request->n_groups, request->which_mask};
}

template <typename Rule>
void hist_buckets_launch(mdb_ctx *ctx, const char *name, const DevSegments &s, const uint32_t *groups, const BucketRequest &r,
                         const Rule &rule, unsigned long long *cells, const HistSlots &slots, unsigned int *words) {
    LaunchTimer timer(ctx, name);
    hipLaunchKernelGGL(k_hist_buckets<Rule>, dim3(hist_blocks(s.n)), dim3(HIST_THREADS), 0, ctx->stream, s, groups, r, rule,
                       cells, slots.offsets, slots.slots, words);
}

int hist_buckets_error(unsigned int error) {
    if (error & ERR_HIST_GROUP) return fail("A group id is not below n_groups.");
    if (error) return fail(describe_error(error));
    return 0;
}

// One pass: the points of the device batch `in` (groups: a device array or nullptr) the request holds, counted into
// zeroed scratch cells and then ADDED to dev_counts (a device array) or host_counts (the caller's, after one download) -
// only once the pass is known to be free of errors.
int hist_buckets_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_bucket_request *request,
                     const std::vector<int32_t> &edge_keys, uint64_t n_rows, unsigned long long *dev_counts,
                     uint64_t *host_counts) {
    const uint64_t n = in->n;
    if (n == 0 || n_rows == 0) return 0;
    const BucketRequest r = bucket_request_of(request);
    const uint64_t total = n_rows * (edge_keys.size() + 1);
    if (hist_buckets_fits(total * 8, "n_groups * n_buckets * n_cells counters")) return 1;
    const DevSegments s = to_dev(in);
    HistSlots slots;
    if (hist_buckets_slots(ctx, in, s, r, &slots)) return 1;
    void *p = nullptr;
    const uint64_t cells_bytes = align_up(total * 8, 256), keys_bytes = align_up(edge_keys.size() * 4, 256);
    if (scratch_reserve(ctx, SCRATCH_HIST_CELLS, cells_bytes + keys_bytes + 256, &p)) return 1;
    Carver scratch(p);
    unsigned long long *cells = scratch.take<unsigned long long>(total);
    int32_t *keys = scratch.take<int32_t>(edge_keys.size());
    unsigned int *words = scratch.take<unsigned int>(2);
    MDB_HIP_CHECK(hipMemsetAsync(cells, 0, total * 8, ctx->stream));
    MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
    MDB_HIP_CHECK(mail_write(ctx, keys, edge_keys.data(), edge_keys.size() * 4));
    if (groups) hist_groups_launch(ctx, groups, n, r.n_groups, words);
    hist_buckets_launch(ctx, "k_hist_buckets", s, groups, r, EdgeRule{keys, (uint32_t)edge_keys.size()}, cells, slots, words);
    unsigned int error = 0;
    MDB_HIP_CHECK(hipMemcpyAsync(&error, words, 4, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (hist_buckets_error(error)) return 1;
    if (host_counts) {
        std::vector<uint64_t> added(total);
        MDB_HIP_CHECK(hipMemcpyAsync(added.data(), cells, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (uint64_t j = 0; j < total; j++) host_counts[j] += added[j];
        return 0;
    }
    hist_fold_launch(ctx, cells, total, dev_counts);
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    return 0;
}

// The order statistics of every (group, bucket) cell of the device batch `in`: SELECT_PASSES passes of k_hist_buckets
// with windows, each followed by k_quantile_select; the outputs are written once everything has succeeded.
int quantile_buckets_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_bucket_request *request,
                         const double *q, uint32_t n_q, uint64_t n_rows, float *out_lo, float *out_hi, uint64_t *n_points) {
    const uint64_t n = in->n;
    if (n_rows == 0) return 0;
    if (n == 0) {
        for (uint64_t row = 0; row < n_rows; row++) n_points[row] = 0;
        return 0;
    }
    const BucketRequest r = bucket_request_of(request);
    const uint32_t n_ranks = 2 * n_q;
    const uint64_t lanes = n_rows * n_ranks, windows = lanes * SELECT_DIGITS;
    if (hist_buckets_fits(windows * 8 + lanes * 12 + n_rows * 8, "n_groups * n_buckets * 2 n_q windows of 256 counters")) return 1;
    const DevSegments s = to_dev(in);
    HistSlots slots;
    if (hist_buckets_slots(ctx, in, s, r, &slots)) return 1;
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_HIST_CELLS, align_up(windows * 8, 256) + align_up(lanes * 8, 256) + align_up(n_rows * 8, 256) +
                                                     align_up(lanes * 4, 256) + 256, &p))
        return 1;
    Carver scratch(p);
    unsigned long long *cells = scratch.take<unsigned long long>(windows);
    unsigned long long *remaining = scratch.take<unsigned long long>(lanes);
    unsigned long long *counted = scratch.take<unsigned long long>(n_rows);
    uint32_t *prefixes = scratch.take<uint32_t>(lanes);
    unsigned int *words = scratch.take<unsigned int>(2);
    SelectQ wanted = {};
    for (uint32_t k = 0; k < n_q; k++) wanted.q[k] = q[k];
    MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
    if (groups) hist_groups_launch(ctx, groups, n, r.n_groups, words);
    for (uint32_t pass = 0; pass < SELECT_PASSES; pass++) {
        const uint32_t pass_ranks = pass == 0 ? 1u : n_ranks;
        MDB_HIP_CHECK(hipMemsetAsync(cells, 0, n_rows * pass_ranks * SELECT_DIGITS * 8, ctx->stream));
        hist_buckets_launch(ctx, "k_hist_buckets_window", s, groups, r,
                            WindowRule{pass == 0 ? nullptr : prefixes, pass_ranks, select_shift(pass)}, cells, slots, words);
        if (pass == 0) { // (every pass would find the same errors: the later ones are not run on a bad batch)
            unsigned int error = 0;
            MDB_HIP_CHECK(hipMemcpyAsync(&error, words, 4, hipMemcpyDeviceToHost, ctx->stream));
            MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            MDB_HIP_CHECK(hipGetLastError());
            if (hist_buckets_error(error)) return 1;
        }
        LaunchTimer timer(ctx, "k_quantile_select");
        hipLaunchKernelGGL(k_quantile_select, dim3((uint32_t)((lanes + HIST_THREADS - 1) / HIST_THREADS)), dim3(HIST_THREADS), 0,
                           ctx->stream, cells, n_rows, n_ranks, pass, wanted, counted, remaining, prefixes);
    }
    std::vector<uint64_t> host_counted(n_rows);
    std::vector<uint32_t> host_keys(lanes);
    unsigned int error = 0;
    MDB_HIP_CHECK(hipMemcpyAsync(host_counted.data(), counted, n_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipMemcpyAsync(host_keys.data(), prefixes, lanes * 4, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipMemcpyAsync(&error, words, 4, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (hist_buckets_error(error)) return 1;
    for (uint64_t row = 0; row < n_rows; row++) {
        n_points[row] = host_counted[row];
        if (host_counted[row] == 0) continue;
        for (uint32_t k = 0; k < n_q; k++) {
            out_lo[row * n_q + k] = hist_float_of_key(select_key_of_ukey(host_keys[row * n_ranks + 2 * k]));
            out_hi[row * n_q + k] = hist_float_of_key(select_key_of_ukey(host_keys[row * n_ranks + 2 * k + 1]));
        }
    }
    return 0;
}

int quantile_buckets_arguments_check(const double *q, uint32_t n_q) {
    if (n_q < 1 || n_q > MDB_QUANTILE_BUCKETS_MAX_Q)
        return fail("n_q must be 1 .. " + std::to_string(MDB_QUANTILE_BUCKETS_MAX_Q) + ".");
    for (uint32_t k = 0; k < n_q; k++)
        if (!(q[k] >= 0.0 && q[k] <= 1.0)) return fail("q must lie in [0, 1].");
    return 0;
}

} // namespace

} // namespace mdb

using namespace mdb;

extern "C" {

int mdb_hist_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                         const mdb_bucket_request *request, const float *edges, uint32_t n_edges, uint64_t *counts) {
    if (!ctx || !in || !request || !edges || !counts) return fail("ctx, in, request, edges and counts must not be NULL.");
    std::vector<int32_t> edge_keys;
    uint64_t n_rows = 0;
    if (hist_edge_keys(edges, n_edges, &edge_keys)) return 1;
    if (hist_buckets_request_check(request, (uint64_t)n_edges + 1, "mdb_hist_buckets*", &n_rows)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return hist_buckets_run(ctx, in, group_of_segment, request, edge_keys, n_rows,
                            reinterpret_cast<unsigned long long *>(counts), nullptr);
}

int mdb_hist_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                          uint32_t n_inputs, const mdb_bucket_request *request, const float *edges, uint32_t n_edges,
                          uint64_t *counts) {
    if (!ctx || !inputs || !request || !edges || !counts)
        return fail("ctx, inputs, request, edges and counts must not be NULL.");
    std::vector<int32_t> edge_keys;
    uint64_t n_rows = 0;
    if (hist_edge_keys(edges, n_edges, &edge_keys)) return 1;
    if (hist_buckets_request_check(request, (uint64_t)n_edges + 1, "mdb_hist_buckets*", &n_rows)) return 1;
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || n_rows == 0) return 0;
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, true)) return 1;
    return hist_buckets_run(ctx, list.segments(), list.groups(), request, edge_keys, n_rows, nullptr, counts);
}

int mdb_hist_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                     const mdb_bucket_request *request, const float *edges, uint32_t n_edges, uint64_t *counts) {
    if (!in) return fail("ctx, in, request, edges and counts must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_hist_buckets_list(ctx, &in, groups, 1, request, edges, n_edges, counts);
}

int mdb_quantile_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                             const mdb_bucket_request *request, const double *q, uint32_t n_q, float *out_lo,
                             float *out_hi, uint64_t *n_points) {
    if (!ctx || !in || !request || !q || !out_lo || !out_hi || !n_points)
        return fail("ctx, in, request, q, out_lo, out_hi and n_points must not be NULL.");
    uint64_t n_rows = 0;
    if (quantile_buckets_arguments_check(q, n_q)) return 1;
    if (hist_buckets_request_check(request, (uint64_t)2 * n_q * SELECT_DIGITS, "mdb_quantile_buckets*", &n_rows)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return quantile_buckets_run(ctx, in, group_of_segment, request, q, n_q, n_rows, out_lo, out_hi, n_points);
}

int mdb_quantile_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                         const mdb_bucket_request *request, const double *q, uint32_t n_q, float *out_lo, float *out_hi,
                         uint64_t *n_points) {
    if (!ctx || !in || !request || !q || !out_lo || !out_hi || !n_points)
        return fail("ctx, in, request, q, out_lo, out_hi and n_points must not be NULL.");
    uint64_t n_rows = 0;
    if (quantile_buckets_arguments_check(q, n_q)) return 1;
    if (hist_buckets_request_check(request, (uint64_t)2 * n_q * SELECT_DIGITS, "mdb_quantile_buckets*", &n_rows)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    if (in->n == 0 || n_rows == 0) return quantile_buckets_run(ctx, in, nullptr, request, q, n_q, n_rows, out_lo, out_hi, n_points);
    // (uploaded once: every pass reads the resident copy)
    mdb_segments_owned *dev = nullptr;
    if (upload_segments_locked(ctx, in, true, &dev)) return 1;
    const uint32_t *groups = nullptr;
    const uint32_t *const host_groups[1] = {group_of_segment};
    const uint64_t rows[1] = {in->n};
    int rc = upload_groups(ctx, host_groups, rows, 1, in->n, &groups);
    if (!rc) rc = quantile_buckets_run(ctx, &dev->seg, groups, request, q, n_q, n_rows, out_lo, out_hi, n_points);
    mdb_segments_free(dev);
    return rc;
}

} // extern "C"
