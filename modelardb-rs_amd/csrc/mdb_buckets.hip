// mdb_buckets.hip - COUNT / MIN / MAX / SUM per date_bin bucket and group, computed on segments.
//
// What the reference answers for SELECT <tags>, date_bin(width, ts, origin), AGG(field) ... GROUP BY 1, 2 with
// GridExec + the date_bin / range filter + AggregateExec (its model-based rule only takes an empty GROUP BY,
// crates/modelardb_storage/src/optimizer/model_simple_aggregates.rs:219), without materialising a point. The range
// aggregate (mdb_agg.hip, k_agg_range) is the one-bucket case: every (segment, bucket) pair below is one call of its
// segment_range, or - for segments whose points live in a bit stream - one stretch of a single decode.
//
//   k_agg_bucket_span      1 lane / segment: how many buckets the segment reaches (from start_time / end_time alone,
//                          clipped by [t_lo, t_hi] and buckets 0 .. n_buckets-1), and its group id checked. A scan
//                          (mdb_scan.hpp) makes pair offsets; one read-back sizes the work.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS pairs (bounded scratch), slices folded in order:
//   k_agg_bucket_partials  1 lane / segment with pairs in the slice: {f64 sum, count, min, max} and the cell key
//                          group * n_buckets + b of each of its pairs. PMC-Mean / Swing on regular timestamps: O(1)
//                          per pair (segment_range's closed forms, its tail decode for residuals). MacaqueV values or
//                          irregular timestamps: the stream is decoded once, a partial flushed at each bucket edge -
//                          unless the stream is in the batch's cursor index (regular timestamps: MacaqueV values, the
//                          residual tails of PMC-Mean / Swing): then k_agg_bucket_pieces decodes it one
//                          lane per piece of 64 values and writes one entry {key, partial} per bucket a piece reaches;
//                          the entries are reduced and folded like the pairs, in slices behind them.
//   k_agg_bucket_check     are the keys non-decreasing in pair order (ModelarDB's storage order: segments by tags, then
//                          start_time, groups following the tags)? If not, a stable radix sort by key (rocPRIM).
//   k_agg_bucket_tree      (k_bucket_tree<AggFoldOps>) runs of equal keys reduced through a fixed tree of 64-entry
//                          tiles: level l+1 holds, per tile of level l, its last key and the fold of the run that ends
//                          the tile.
//   k_agg_bucket_fold      (k_bucket_fold<AggFoldOps>) 1 lane / pair: the lane of a run's last pair folds the run (its
//                          tile, then one tile's entry per level up) and merges it into the cell - no two lanes write
//                          one cell, no float atomics, the order of every addition fixed by the pair order: run-to-run
//                          deterministic.
// The tree and the fold are one template for every per-bucket operator (mdb_bucket_fold.hpp: the two kernels, the
// scratch of a slice, the working copy of the cells); what is the aggregates' own is AggFoldOps below.
// Bytes (Swing on regular timestamps): ~70 B of metadata per segment read, 32 B per pair written and read back.
#include "mdb_bucket_fold.hpp"
#include "mdb_scan.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <vector>

namespace mdb {

__global__ __launch_bounds__(BUCKET_THREADS) void k_agg_bucket_span(DevSegments s, const uint32_t *__restrict__ groups,
                                                                    BucketRequest r,
                                                                    unsigned long long *__restrict__ counts,
                                                                    unsigned int *__restrict__ error) {
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= s.n) return;
    uint64_t first = 0;
    uint64_t count = bucket_span(s.start_time[i], s.end_time[i], r, &first);
    if (groups && groups[i] >= r.n_groups) {
        atomicOr(error, ERR_BUCKET_GROUP);
        count = 0;
    }
    counts[i] = count;
}

// The pairs of a segment whose points are a bit stream (MacaqueV values, irregular timestamps): slots [j0, j1) of the
// slice, buckets b_first + (j - off). Pass 1 leaves each slot's index interval [k_lo, k_hi] of points in its sum
// field (k_lo > k_hi: no point); pass 2 decodes the values once, each into the slot whose interval holds it, and
// overwrites every slot with its partial. Returns false when the timestamps turn out not to be sorted (a malformed
// stream): the caller then overwrites the slots with segment_range pair by pair, which tests every point. `pred` (a
// selector by value: rows are not counted here) is tested where a point is accumulated, nowhere else: the slots, the
// decode and the tail's seed are the unfiltered ones.
template <typename Pred>
__device__ bool bucket_stream_partials(const DevSegments &s, uint64_t i, const SegInfo &info, const BucketRequest &r,
                                       uint64_t off, uint64_t b_first, uint64_t j0, uint64_t j1, uint64_t p0,
                                       BucketPartial *__restrict__ out, uint32_t *error, const Pred &pred) {
    static_assert(!Pred::by_row, "the buckets select by value: rows are not threaded through them");
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint32_t n_res = d.n_total - d.n_model;
    auto interval = [&](uint64_t j) -> uint2 * { return reinterpret_cast<uint2 *>(&out[j - p0].sum); };
    uint32_t needed = 0; // points [0, needed) reach a slot
    if (d.flags & FLAG_REGULAR) {
        for (uint64_t j = j0; j < j1; j++) {
            int64_t lo, hi;
            bucket_bounds(r, b_first + (j - off), &lo, &hi);
            uint32_t k_lo = 1, k_hi = 0;
            if (regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi)) needed = k_hi + 1;
            else k_lo = 1, k_hi = 0;
            *interval(j) = make_uint2(k_lo, k_hi);
        }
    } else {
        for (uint64_t j = j0; j < j1; j++) *interval(j) = make_uint2(1, 0);
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
                                            if (slot != ~0ull) *interval(slot) = make_uint2(k_lo, k_hi);
                                            slot = j;
                                            k_lo = k;
                                        }
                                        k_hi = k;
                                    });
        if (!sorted) return false;
        if (slot != ~0ull) {
            *interval(slot) = make_uint2(k_lo, k_hi);
            needed = k_hi + 1;
        }
    }

    // Pass 2: the points in index order; slot j's interval is read before its partial overwrites it.
    uint64_t j = j0;
    uint2 current = *interval(j);
    RangeAcc acc;
    auto flush = [&]() {
        out[j - p0] = BucketPartial{acc.sum, acc.count, acc.min, acc.max};
        acc = RangeAcc();
        j++;
        if (j < j1) current = *interval(j);
    };
    auto visit = [&](uint32_t k, float v) {
        while (j < j1 && k > current.y) flush();
        if (j < j1 && k >= current.x && pred.counts(v, 0)) acc.point(v);
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
    return true;
}

// Pred: AllValues for mdb_agg_buckets*, ValueKeys for mdb_agg_buckets_filter* (which points of a pair count; the pairs,
// keys and decodes are the same).
template <typename Pred>
__global__ __launch_bounds__(BUCKET_THREADS) void k_agg_bucket_partials(DevSegments s,
                                                                        const uint32_t *__restrict__ groups,
                                                                        BucketRequest r,
                                                                        const unsigned long long *__restrict__ offsets,
                                                                        uint64_t p0, uint64_t p1,
                                                                        BucketPartial *__restrict__ out,
                                                                        unsigned long long *__restrict__ keys,
                                                                        unsigned int *__restrict__ error_out,
                                                                        const unsigned long long *__restrict__ piece_base,
                                                                        Pred pred) {
    static_assert(!Pred::by_row, "the buckets select by value: rows are not threaded through them");
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= s.n) return;
    const uint64_t off = offsets[i], stop = offsets[i + 1];
    const uint64_t j0 = off > p0 ? off : p0, j1 = stop < p1 ? stop : p1;
    if (j0 >= j1) return;
    uint64_t b_first = 0;
    (void)bucket_span(s.start_time[i], s.end_time[i], r, &b_first);
    const uint64_t row = (uint64_t)(groups ? groups[i] : 0u) * r.n_buckets;
    for (uint64_t j = j0; j < j1; j++) keys[j - p0] = row + b_first + (j - off);
    SegInfo info = analyse_segment(s, i);
    uint32_t error = info.error;
    if (!error && bucket_values_by_pieces(s, i, info, piece_base)) {
        // (every point is k_agg_bucket_pieces': the pairs stay empty)
        for (uint64_t j = j0; j < j1; j++) out[j - p0] = bucket_empty();
    } else if (!error) {
        const bool tail_by_pieces = bucket_tail_by_pieces(s, i, info, piece_base); // (the model's points only, then)
        const bool stream = !(info.desc.flags & FLAG_REGULAR) || (info.desc.flags & FLAG_TYPE_MASK) == MDB_MACAQUE_V_ID;
        if (!stream || !bucket_stream_partials(s, i, info, r, off, b_first, j0, j1, p0, out, &error, pred)) {
            for (uint64_t j = j0; j < j1; j++) {
                int64_t lo, hi;
                bucket_bounds(r, b_first + (j - off), &lo, &hi);
                RangeAcc acc;
                segment_range(s, i, info, lo, hi, acc, &error, tail_by_pieces, pred);
                out[j - p0] = BucketPartial{acc.sum, acc.count, acc.min, acc.max};
            }
        }
    }
    if (error) atomicOr(error_out, error);
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_agg_bucket_check(const unsigned long long *__restrict__ keys,
                                                                     uint64_t n, unsigned int *__restrict__ unsorted) {
    const uint64_t j = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x + 1;
    // (the flag is read first: keys that descend everywhere - the runs of mdb_binned_buckets* - then cost the few
    // atomics of the waves that run before the first one lands, not one per wave)
    if (j < n && keys[j] < keys[j - 1] && *(volatile const unsigned int *)unsorted == 0) atomicOr(unsorted, 1u);
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_agg_bucket_iota(uint32_t *__restrict__ out, uint64_t n) {
    const uint64_t j = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (j < n) out[j] = (uint32_t)j;
}

// What the tree and fold (mdb_bucket_fold.hpp) need to know of the aggregates: a run enters its cell by mdb_agg_merge's
// rules, for the aggregates in which_mask.
struct AggFoldOps : FoldOps<BucketPartial, mdb_agg_state> {
    static constexpr const char *tree_name = "k_agg_bucket_tree", *fold_name = "k_agg_bucket_fold";
    uint32_t which_mask;
    __device__ __forceinline__ static BucketPartial empty() { return bucket_empty(); }
    __device__ __forceinline__ static void merge(BucketPartial &into, const BucketPartial &from) { bucket_add(into, from); }
    __device__ __forceinline__ static bool is_empty(const BucketPartial &acc) { return acc.count == 0; }
    __device__ __forceinline__ void apply(mdb_agg_state &cell, const BucketPartial &acc) const {
        if (which_mask & (MDB_AGG_COUNT | MDB_AGG_AVG)) cell.count += acc.count;
        if (which_mask & (MDB_AGG_SUM | MDB_AGG_AVG)) cell.sum += acc.sum;
        if ((which_mask & MDB_AGG_MIN) && !(acc.min != acc.min) && (cell.min != cell.min || acc.min < cell.min))
            cell.min = acc.min;
        if ((which_mask & MDB_AGG_MAX) && !(acc.max != acc.max) && (cell.max != cell.max || acc.max > cell.max))
            cell.max = acc.max;
    }
};

// ---- the pieces of MacaqueV streams ----------------------------------------------------------------------------
// The streams bucket_values_by_pieces / bucket_tail_by_pieces take (regular timestamps: point k at start + k delta)
// are aggregated like k_agg_mv_range does under a time range - one lane per piece of 64 values, every lane decoding
// in every step - but each lane flushes a partial at every bucket edge: ENTRIES {key, partial}, one per bucket its
// visible values reach (empty ones included), at offsets a count per piece and a scan have given. Entries of one
// stream follow each other in key order; buckets_run reduces and folds them like its (segment, bucket) pairs.

// (bucket_piece_span, the visible values of a piece and the buckets they reach: mdb_buckets.hpp)
__global__ __launch_bounds__(256) void k_agg_bucket_piece_count(DevSegments s, BucketRequest r,
                                                                 const unsigned long long *__restrict__ piece_base,
                                                                 const MvCursor *__restrict__ cursors, unsigned long long n_pieces,
                                                                 unsigned long long *__restrict__ counts) {
    const unsigned long long piece = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (piece >= n_pieces) return;
    SegInfo info;
    uint32_t from, upto;
    uint64_t b_first, b_last;
    counts[piece] = bucket_piece_span(s, r, piece_base, load_piece_cursor(cursors, piece), &info, &from, &upto, &b_first, &b_last)
                        ? b_last - b_first + 1 : 0;
}

// Writes the entries [e0, e1) of the call (entry e at e - e0). Pred (AllValues, or the ValueKeys of
// mdb_agg_buckets_filter*) says which decoded values are accumulated: the entries, and the decode, stay the same.
template <typename Pred>
__global__ __launch_bounds__(MDB_WAVE) void k_agg_bucket_pieces(DevSegments s, BucketRequest r, const uint32_t *__restrict__ groups,
                                                                const unsigned long long *__restrict__ piece_base,
                                                                const MvCursor *__restrict__ cursors, unsigned long long n_pieces,
                                                                const unsigned long long *__restrict__ offsets,
                                                                unsigned long long e0, unsigned long long e1,
                                                                unsigned long long *__restrict__ keys,
                                                                BucketPartial *__restrict__ out, Pred pred) {
    static_assert(!Pred::by_row, "the buckets select by value: rows are not threaded through them");
    __shared__ uint32_t ring[PIECE_RING_ROWS][MDB_WAVE];
    const int lane = threadIdx.x;
    const unsigned long long piece = (unsigned long long)blockIdx.x * MDB_WAVE + lane;
    const uint8_t *values_first = first_buffer(s.values), *residuals_first = first_buffer(s.residuals); // (see view_data())
    uint32_t to_decode = 0, to_skip = 0, point_index = 0;
    uint64_t b_first = 0, b_last = 0, base = 0, row = 0;
    int64_t start = 0, delta = 0;
    PieceReader reader;
    PieceState state = piece_state_idle();
    reader.idle(cursors);
    if (piece < n_pieces && offsets[piece + 1] > e0 && offsets[piece] < e1) {
        const PieceCursor cursor = load_piece_cursor(cursors, piece);
        SegInfo info;
        uint32_t from, upto;
        if (bucket_piece_span(s, r, piece_base, cursor, &info, &from, &upto, &b_first, &b_last)) {
            point_index = cursor.point_index();
            // (a tail is XOR-seeded with the model's last RECONSTRUCTED value, models/mod.rs:241-249: what grid() sees)
            const uint32_t seed = cursor.residual() ? __float_as_uint(info.desc.value) : 0u;
            to_decode = upto - point_index;
            to_skip = from - point_index;
            start = info.desc.start;
            delta = info.desc.delta;
            base = offsets[piece];
            row = (uint64_t)(groups ? groups[cursor.segment()] : 0u) * r.n_buckets;
            piece_open(reader, s, cursor, values_first, residuals_first);
            state = piece_state(cursor, seed);
        }
    }
    if (!__any(to_decode > 0)) return;
    RangeAcc acc;
    uint64_t bucket = b_first;
    auto flush = [&]() {
        const uint64_t e = base + (bucket - b_first);
        if (e >= e0 && e < e1) {
            keys[e - e0] = row + bucket;
            out[e - e0] = BucketPartial{acc.sum, acc.count, acc.min, acc.max};
        }
        acc = RangeAcc();
        bucket++;
    };
    auto take = [&](uint32_t k, uint32_t bits) {
        if (k < to_skip || k >= to_decode) return;
        const int64_t t = start + (int64_t)((uint64_t)(point_index + k) * (uint64_t)delta);
        const uint64_t b = ((uint64_t)t - (uint64_t)r.origin) / (uint64_t)r.width;
        while (bucket < b) flush();
        if (pred.counts(__uint_as_float(bits), 0)) acc.point(__uint_as_float(bits)); // (by value: Pred::by_row is false)
    };
    piece_start(reader, ring, lane);
    for (uint32_t k = 0, most = wave_max_u32(to_decode); k < most; k += 2) {
        if (__any(reader.hungry())) reader.top_up(ring, lane);
        const uint32_t even = piece_decode_value(reader, state, ring, lane);
        const uint32_t odd = piece_decode_value(reader, state, ring, lane);
        take(k, even);
        take(k + 1, odd);
    }
    if (to_decode > 0) flush(); // (bucket == b_last)
}

// The entries of the pieces taken above. bucket_pieces_count sizes them (offsets: per piece of the index, n_pieces + 1,
// in scratch); bucket_pieces_entries writes the entries [e0, e1) to keys / out (at e - e0), with the values that pass
// `filter` only (nullptr: every value; the entries are the same either way).
int bucket_pieces_count(mdb_ctx *ctx, const DevSegments &s, const BucketRequest &r, const unsigned long long *piece_base,
                        const MvIndex &index, const unsigned long long **offsets_out, unsigned long long *total) {
    *total = 0;
    const uint64_t n = index.n_pieces;
    void *p = nullptr;
    const uint64_t counts_bytes = align_up(n * 8, 256), offsets_bytes = align_up((n + 1) * 8, 256);
    if (scratch_reserve(ctx, SCRATCH_BUCKET_PIECES, counts_bytes + offsets_bytes + scan_block_sums_bytes(n) + 256, &p))
        return 1;
    unsigned long long *counts = static_cast<unsigned long long *>(p);
    unsigned long long *offsets = reinterpret_cast<unsigned long long *>(static_cast<char *>(p) + counts_bytes);
    unsigned long long *block_sums = reinterpret_cast<unsigned long long *>(static_cast<char *>(p) + counts_bytes + offsets_bytes);
    {
        LaunchTimer timer(ctx, "k_agg_bucket_piece_count");
        hipLaunchKernelGGL(k_agg_bucket_piece_count, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, s, r,
                           piece_base, static_cast<const MvCursor *>(index.cursors), (unsigned long long)n, counts);
    }
    if (device_exclusive_scan(ctx, ItemsOf<unsigned long long>{counts}, n, offsets, block_sums, "k_agg_bucket_piece_count")) return 1;
    MDB_HIP_CHECK(hipMemcpyAsync(total, offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    *offsets_out = offsets;
    return 0;
}

static int bucket_pieces_entries(mdb_ctx *ctx, const DevSegments &s, const BucketRequest &r, const uint32_t *groups,
                                 const unsigned long long *piece_base, const MvIndex &index, const unsigned long long *offsets,
                                 unsigned long long e0, unsigned long long e1, unsigned long long *keys, BucketPartial *out,
                                 const ValueKeys *filter) {
    const uint64_t n = index.n_pieces;
    const dim3 blocks((uint32_t)((n + MDB_WAVE - 1) / MDB_WAVE));
    const MvCursor *cursors = static_cast<const MvCursor *>(index.cursors);
    if (filter) {
        LaunchTimer timer(ctx, "k_agg_bucket_pieces_filter");
        hipLaunchKernelGGL(k_agg_bucket_pieces<ValueKeys>, blocks, dim3(MDB_WAVE), 0, ctx->stream, s, r, groups,
                           piece_base, cursors, (unsigned long long)n, offsets, e0, e1, keys, out, *filter);
    } else {
        LaunchTimer timer(ctx, "k_agg_bucket_pieces");
        hipLaunchKernelGGL(k_agg_bucket_pieces<AllValues>, blocks, dim3(MDB_WAVE), 0, ctx->stream, s, r, groups,
                           piece_base, cursors, (unsigned long long)n, offsets, e0, e1, keys, out, AllValues());
    }
    return 0;
}

// ---- the host steps mdb_m4.hip shares (mdb_buckets.hpp) --------------------------------------------------------

int bucket_span_pairs(mdb_ctx *ctx, const mdb_segments *in, const DevSegments &s, const uint32_t *groups,
                      const BucketRequest &r, const unsigned long long **offsets_out, unsigned int **words_out,
                      unsigned long long *total_out, const BucketSpanKernel *span_kernel) {
    const uint64_t n = in->n;
    // Span: pair offsets and the read-back words (total pairs, error, unsorted).
    void *p;
    const uint64_t offsets_bytes = align_up((n + 1) * 8, 256), sums_bytes = align_up(scan_block_sums_bytes(n), 256);
    if (scratch_reserve(ctx, SCRATCH_BUCKET_SPAN, 2 * offsets_bytes + sums_bytes + 256, &p)) return 1;
    Carver span(p);
    unsigned long long *counts = span.take<unsigned long long>(n + 1);
    unsigned long long *offsets = span.take<unsigned long long>(n + 1);
    unsigned long long *block_sums = span.take<unsigned long long>(scan_block_sums_bytes(n) / 8);
    unsigned int *words = span.take<unsigned int>(2);
    MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
    if (span_kernel) {
        LaunchTimer timer(ctx, span_kernel->name);
        span_kernel->launch(ctx, s, groups, r, counts, words, span_kernel->arg);
    } else {
        LaunchTimer timer(ctx, "k_agg_bucket_span");
        hipLaunchKernelGGL(k_agg_bucket_span, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, r,
                           counts, words);
    }
    if (device_exclusive_scan(ctx, ItemsOf<unsigned long long>{counts}, n, offsets, block_sums, "k_agg_bucket_scan")) return 1;
    unsigned long long total = 0;
    unsigned int span_error = 0;
    MDB_HIP_CHECK(hipMemcpyAsync(&total, offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipMemcpyAsync(&span_error, words, 4, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (span_error & ERR_BUCKET_GROUP) return fail("A group id is not below n_groups.");
    *offsets_out = offsets;
    *words_out = words;
    *total_out = total;
    return 0;
}

void bucket_keys_check(mdb_ctx *ctx, const unsigned long long *keys, uint64_t m, unsigned int *unsorted) {
    if (m <= 1) return;
    LaunchTimer timer(ctx, "k_agg_bucket_check");
    hipLaunchKernelGGL(k_agg_bucket_check, dim3(blocks_for(m - 1)), dim3(BUCKET_THREADS), 0, ctx->stream, keys, m,
                       unsorted);
}

int bucket_slice_check(mdb_ctx *ctx, const unsigned long long *keys, uint64_t m, unsigned int *words,
                       unsigned int *error, bool *unsorted) {
    bucket_keys_check(ctx, keys, m, words + 1);
    unsigned int read_back[2] = {0, 0};
    MDB_HIP_CHECK(hipMemcpyAsync(read_back, words, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    *error = read_back[0];
    *unsorted = read_back[1] != 0;
    return 0;
}

int bucket_keys_sort(mdb_ctx *ctx, unsigned long long *keys, uint64_t m, unsigned int key_bits,
                     const unsigned long long **sorted_out, const uint32_t **order_out) {
    void *p;
    const uint64_t keys_bytes = align_up(m * 8, 256), order_bytes = align_up(m * 4, 256);
    size_t sort_bytes = 0;
    MDB_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, keys, static_cast<uint32_t *>(nullptr),
                                            static_cast<uint32_t *>(nullptr), (size_t)m, 0u, key_bits, ctx->stream));
    if (scratch_reserve(ctx, SCRATCH_BUCKET_SORT, keys_bytes + 2 * order_bytes + sort_bytes, &p)) return 1;
    Carver sort_scratch(p);
    unsigned long long *sorted_keys = sort_scratch.take<unsigned long long>(m);
    uint32_t *order_in = sort_scratch.take<uint32_t>(m);
    uint32_t *order = sort_scratch.take<uint32_t>(m);
    void *sort_storage = sort_scratch.at;
    LaunchTimer timer(ctx, "k_agg_bucket_sort");
    hipLaunchKernelGGL(k_agg_bucket_iota, dim3(blocks_for(m)), dim3(BUCKET_THREADS), 0, ctx->stream, order_in, m);
    MDB_HIP_CHECK(rocprim::radix_sort_pairs(sort_storage, sort_bytes, keys, sorted_keys, order_in, order, (size_t)m,
                                            0u, key_bits, ctx->stream));
    *sorted_out = sorted_keys;
    *order_out = order;
    return 0;
}

uint64_t slice_pairs_setting() {
    if (const char *text = option_text("MDB_AGG_BUCKET_SLICE_PAIRS")) {
        const long long value = std::atoll(text);
        if (value >= 1) return std::min<uint64_t>((uint64_t)value, BUCKET_SLICE_MAX);
    }
    return BUCKET_SLICE_DEFAULT;
}

// The host-side checks every form makes before it touches the device.
static int bucket_request_check(const mdb_bucket_request *request, uint64_t *n_cells) {
    if (request->width <= 0) return fail("The bucket width must be positive.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    const unsigned __int128 cells = (unsigned __int128)request->n_groups * request->n_buckets;
    if (cells * sizeof(mdb_agg_state) > (unsigned __int128)UINT64_MAX)
        return fail("n_groups * n_buckets overflows.");
    *n_cells = (uint64_t)cells;
    return 0;
}

// The buckets of the device batch `in` (groups: a device array or nullptr) folded into `cells_target`, a device array
// of n_cells states. `host_cells` (host forms): the caller's array, which is uploaded, folded and downloaded instead;
// either way nothing of the caller's is written unless the whole call succeeds. `filter` (nullptr: every value) is the
// value predicate of mdb_agg_buckets_filter*: only k_agg_bucket_partials and k_agg_bucket_pieces see it.
int buckets_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_bucket_request *request,
                uint64_t n_cells, mdb_agg_state *dev_cells, mdb_agg_state *host_cells,
                const ValueKeys *filter = nullptr) {
    const uint64_t n = in->n;
    if (n == 0 || request->n_buckets == 0) return 0;
    const BucketRequest r = {request->origin, request->width, request->n_buckets, request->t_lo, request->t_hi,
                             request->n_groups, request->which_mask};
    if (n > UINT64_MAX / request->n_buckets)
        return fail("Too many (segment, bucket) pairs for one call: split the batch.");
    const DevSegments s = to_dev(in);

    const unsigned long long *offsets = nullptr;
    unsigned int *words = nullptr;
    unsigned long long total = 0;
    if (bucket_span_pairs(ctx, in, s, groups, r, &offsets, &words, &total)) return 1;
    if (total == 0) return 0;
    // The MacaqueV streams of the batch's cursor index (built here for a batch the library holds; MDB_GRID_MV_INDEX=0:
    // none) go piece by piece: their entries are folded behind the pairs, in slices of their own.
    std::shared_ptr<MvIndex> index;
    const unsigned long long *piece_base = nullptr, *entry_offsets = nullptr;
    unsigned long long entries = 0;
    if (mv_index_for_range(ctx, in, &index, &piece_base)) return 1;
    if (piece_base && bucket_pieces_count(ctx, s, r, piece_base, *index, &entry_offsets, &entries)) return 1;

    const uint64_t slice = slice_pairs_setting();
    const uint64_t pair_slices = (total + slice - 1) / slice, entry_slices = (entries + slice - 1) / slice;
    const uint64_t n_slices = pair_slices + entry_slices;
    const uint64_t cap = std::min<uint64_t>(slice, std::max<uint64_t>(total, entries));
    BucketCells<mdb_agg_state> cells;
    if (cells.stage(ctx, n_cells, dev_cells, host_cells, n_slices)) return 1;
    BucketFold<AggFoldOps> fold(AggFoldOps{{}, r.which_mask});
    if (fold.reserve(ctx, cap, n_cells)) return 1;
    BucketPartial *partials = fold.partials();
    unsigned long long *keys = fold.keys();

    for (uint64_t k = 0; k < n_slices; k++) {
        // (slices of pairs first, then slices of the pieces' entries)
        const bool pairs = k < pair_slices;
        const uint64_t p0 = (pairs ? k : k - pair_slices) * slice;
        const uint64_t p1 = std::min<uint64_t>(p0 + slice, pairs ? total : entries), m = p1 - p0;
        MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
        if (pairs && filter) {
            LaunchTimer timer(ctx, "k_agg_bucket_partials_filter");
            hipLaunchKernelGGL(k_agg_bucket_partials<ValueKeys>, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0,
                               ctx->stream, s, groups, r, offsets, p0, p1, partials, keys, words, piece_base, *filter);
        } else if (pairs) {
            LaunchTimer timer(ctx, "k_agg_bucket_partials");
            hipLaunchKernelGGL(k_agg_bucket_partials<AllValues>, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0,
                               ctx->stream, s, groups, r, offsets, p0, p1, partials, keys, words, piece_base,
                               AllValues());
        } else if (bucket_pieces_entries(ctx, s, r, groups, piece_base, *index, entry_offsets, p0, p1, keys, partials,
                                         filter)) {
            return 1;
        }
        unsigned int error = 0;
        bool unsorted = false;
        if (bucket_slice_check(ctx, keys, m, words, &error, &unsorted)) return 1;
        if (error) return fail(describe_error(error));
        if (fold.fold_slice(ctx, m, unsorted, cells.cells())) return 1;
    }
    return cells.commit();
}

// The host-side checks of the filtered forms, before the device is used: the request's and the filter's own, then the
// request with its time range narrowed to the intersection with the filter's (an empty intersection selects nothing
// but still has its group ids checked: buckets_run runs as for any range).
static int bucket_filter_check(const mdb_bucket_request *request, const mdb_value_filter *filter, uint64_t *n_cells,
                               ValueKeys *keys, mdb_bucket_request *narrowed) {
    if (bucket_request_check(request, n_cells) || value_keys_fold(filter, keys)) return 1;
    *narrowed = *request;
    narrowed->t_lo = std::max(request->t_lo, filter->t_lo);
    narrowed->t_hi = std::min(request->t_hi, filter->t_hi);
    return 0;
}

// The group ids of the host forms, uploaded next to the batch (nullptr: every segment in group 0). (mdb_hist.hip too)
int upload_groups(mdb_ctx *ctx, const uint32_t *const *groups, const uint64_t *rows, uint32_t n_inputs,
                         uint64_t n, const uint32_t **out) {
    *out = nullptr;
    bool any = false;
    for (uint32_t k = 0; k < n_inputs; k++) any = any || (groups && groups[k] && rows[k] > 0);
    if (!any || n == 0) return 0;
    void *p;
    if (scratch_reserve(ctx, SCRATCH_BUCKET_GROUPS, n * 4, &p)) return 1;
    uint32_t *dev = static_cast<uint32_t *>(p);
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (groups[k])
            MDB_HIP_CHECK(hipMemcpyAsync(dev + at, groups[k], rows[k] * 4, hipMemcpyHostToDevice, ctx->stream));
        else
            MDB_HIP_CHECK(hipMemsetAsync(dev + at, 0, rows[k] * 4, ctx->stream));
        at += rows[k];
    }
    *out = dev;
    return 0;
}

UploadedSegments::~UploadedSegments() {
    if (y_dev_) mdb_segments_free(y_dev_);
    if (dev_) mdb_segments_free(dev_);
}

const mdb_segments *UploadedSegments::segments() const { return &dev_->seg; }
const mdb_segments *UploadedSegments::y_segments() const { return y_dev_ ? &y_dev_->seg : &dev_->seg; }

static int upload_list_groups(mdb_ctx *ctx, const mdb_segments *const *inputs, uint32_t n_inputs,
                              const uint32_t *const *group_of_segment, const uint32_t **groups) {
    std::vector<uint64_t> rows(n_inputs);
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        rows[k] = inputs[k]->n;
        n += rows[k];
    }
    return upload_groups(ctx, group_of_segment, rows.data(), n_inputs, n, groups);
}

int UploadedSegments::upload(const mdb_segments *const *inputs, uint32_t n_inputs,
                             const uint32_t *const *group_of_segment, bool transient) {
    MDB_HIP_CHECK(hipSetDevice(ctx_->device));
    if (upload_segment_list_locked(ctx_, inputs, n_inputs, transient, &dev_)) return 1;
    return upload_list_groups(ctx_, inputs, n_inputs, group_of_segment, &groups_);
}

int UploadedSegments::upload_pair(const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys, uint32_t n_y,
                                  const uint32_t *const *group_of_segment_x) {
    bool same = n_x == n_y;
    for (uint32_t k = 0; same && k < n_x; k++) same = xs[k] == ys[k];
    MDB_HIP_CHECK(hipSetDevice(ctx_->device));
    // (uploads the library holds: two batches are alive at once)
    if (upload_segment_list_locked(ctx_, xs, n_x, false, &dev_)) return 1;
    if (!same && upload_segment_list_locked(ctx_, ys, n_y, false, &y_dev_)) return 1;
    return upload_list_groups(ctx_, xs, n_x, group_of_segment_x, &groups_);
}

// (the host forms of both calls: `filter` nullptr for mdb_agg_buckets*, else the folded keys and narrowed request)
static int buckets_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                            uint32_t n_inputs, const mdb_bucket_request *request, uint64_t n_cells,
                            const ValueKeys *filter, mdb_agg_state *inout) {
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        n += inputs[k]->n;
    }
    if (n == 0 || request->n_buckets == 0) return 0;
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, false)) return 1;
    return buckets_run(ctx, list.segments(), list.groups(), request, n_cells, nullptr, inout, filter);
}

} // namespace mdb

using namespace mdb;

extern "C" {

int mdb_agg_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                        const mdb_bucket_request *request, mdb_agg_state *inout) {
    if (!ctx || !in || !request || !inout) return fail("ctx, in, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (bucket_request_check(request, &n_cells)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return buckets_run(ctx, in, group_of_segment, request, n_cells, inout, nullptr);
}

int mdb_agg_buckets_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                         uint32_t n_inputs, const mdb_bucket_request *request, mdb_agg_state *inout) {
    if (!ctx || !inputs || !request || !inout) return fail("ctx, inputs, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (bucket_request_check(request, &n_cells)) return 1;
    return buckets_list_run(ctx, inputs, group_of_segment, n_inputs, request, n_cells, nullptr, inout);
}

int mdb_agg_buckets(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                    const mdb_bucket_request *request, mdb_agg_state *inout) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_agg_buckets_list(ctx, &in, groups, 1, request, inout);
}

int mdb_agg_buckets_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                               const mdb_bucket_request *request, const mdb_value_filter *filter,
                               mdb_agg_state *inout) {
    if (!ctx || !in || !request || !filter || !inout)
        return fail("ctx, in, request, filter and inout must not be NULL.");
    uint64_t n_cells = 0;
    ValueKeys keys;
    mdb_bucket_request narrowed;
    if (bucket_filter_check(request, filter, &n_cells, &keys, &narrowed)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return buckets_run(ctx, in, group_of_segment, &narrowed, n_cells, inout, nullptr, &keys);
}

int mdb_agg_buckets_filter_list(mdb_ctx *ctx, const mdb_segments *const *inputs,
                                const uint32_t *const *group_of_segment, uint32_t n_inputs,
                                const mdb_bucket_request *request, const mdb_value_filter *filter,
                                mdb_agg_state *inout) {
    if (!ctx || !inputs || !request || !filter || !inout)
        return fail("ctx, inputs, request, filter and inout must not be NULL.");
    uint64_t n_cells = 0;
    ValueKeys keys;
    mdb_bucket_request narrowed;
    if (bucket_filter_check(request, filter, &n_cells, &keys, &narrowed)) return 1;
    return buckets_list_run(ctx, inputs, group_of_segment, n_inputs, &narrowed, n_cells, &keys, inout);
}

int mdb_agg_buckets_filter(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                           const mdb_bucket_request *request, const mdb_value_filter *filter, mdb_agg_state *inout) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_agg_buckets_filter_list(ctx, &in, groups, 1, request, filter, inout);
}

} // extern "C"
