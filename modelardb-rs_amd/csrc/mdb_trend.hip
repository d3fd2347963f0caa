// mdb_trend.hip - the linear trend of a field over time on segments (mdb_trend_buckets*): per date_bin bucket and group
// one mdb_comoments_cell with x = the time offset of a point inside its bucket and y = its value.
//
// What the reference answers with GridExec -> AggregateExec(regr_slope(field, ts) / regr_r2 / corr / covar_*) over
// every rebuilt point. mdb_comoments_buckets* cannot stand in: its y is a second field column, and a timestamp does
// not fit an f32. Here the time side needs no data at all. The structure is that of mdb_moments.hip with a 48-byte
// partial; the span, scan, key check and sort are shared (mdb_buckets.hpp), and the tree and the fold are the one
// template of every per-bucket operator (mdb_bucket_fold.hpp), instantiated here with mdb_comoments.hpp's
// ComomentsFoldOps - under the names mdb_comoments.hip's launches have:
//
//   k_agg_bucket_span   (shared) the buckets each segment reaches, its group id checked; a scan makes pair offsets.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS pairs, slices folded one after the other:
//   k_trend_partials    1 lane / segment with pairs in the slice: the cell and the cell key of each pair. PMC-Mean on
//                       regular timestamps: O(1), no loop - the x sums of n points are closed forms in n and the
//                       sampling interval. Swing on regular timestamps: the same x side, the y side point by point in
//                       registers, no memory traffic. Residual tails, MacaqueV values, irregular timestamps: decoded
//                       once, the timestamp beside the value (trend_stream_partials). Streams in the batch's cursor
//                       index are left to
//   k_trend_pieces      1 lane / piece of 64 values, one entry {key, cell} per bucket the piece reaches; the entries
//                       are reduced and folded like the pairs, in slices behind them.
//   k_agg_bucket_check  (shared) keys non-decreasing? If not, a stable radix sort by key.
//   k_comoments_tree, k_comoments_fold  (k_bucket_tree / k_bucket_fold<ComomentsFoldOps>) runs of equal keys reduced
//                       and merged into the cells.
// Every run is summed around its first pair (mdb_trend.hpp) and runs meet only in comoments_merge, in an order fixed by
// the input, the request and the slice size: two runs of a call agree bit for bit, and a different order of merges
// moves the five doubles by rounding only. No y column, no strided read, no scratch beyond the pairs.
//
// Scratch layout: 48 B per pair (the cell) and the 8-byte key, written and read back.
#include "mdb_trend.hpp"
#include "mdb_scan.hpp"

#include <algorithm>

namespace mdb {

__global__ __launch_bounds__(BUCKET_THREADS) void k_trend_partials(DevSegments s, const uint32_t *__restrict__ groups,
                                                              BucketRequest r,
                                                              const unsigned long long *__restrict__ offsets,
                                                              uint64_t p0, uint64_t p1,
                                                              mdb_comoments_cell *__restrict__ out,
                                                              unsigned long long *__restrict__ keys,
                                                              unsigned int *__restrict__ error_out,
                                                              const unsigned long long *__restrict__ piece_base) {
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
    if (error || bucket_values_by_pieces(s, i, info, piece_base)) {
        // (an error: the call fails; by pieces: every point is k_trend_pieces' - the pairs stay empty)
        for (uint64_t j = j0; j < j1; j++) out[j - p0] = comoments_empty();
    } else {
        const bool tail_by_pieces = bucket_tail_by_pieces(s, i, info, piece_base); // (the model's points only, then)
        const bool regular = (info.desc.flags & FLAG_REGULAR) != 0;
        const bool stream = !regular || (info.desc.flags & FLAG_TYPE_MASK) == MDB_MACAQUE_V_ID;
        if (!stream) {
            for (uint64_t j = j0; j < j1; j++) {
                const uint64_t b = b_first + (j - off);
                int64_t lo, hi;
                bucket_bounds(r, b, &lo, &hi);
                out[j - p0] = trend_regular_pair(s, i, info, lo, hi, trend_bucket_base(r.origin, r.width, b), &error,
                                                 tail_by_pieces);
            }
        } else if (!trend_stream_partials(s, i, info, r, off, b_first, j0, j1, p0, out, &error)) {
            for (uint64_t j = j0; j < j1; j++) {
                int64_t lo, hi;
                bucket_bounds(r, b_first + (j - off), &lo, &hi);
                trend_unsorted_pair(s, i, info, r, off, b_first, lo, hi, j, p0, out, &error);
            }
        }
    }
    if (error) atomicOr(error_out, error);
}

// The pieces of the MacaqueV streams bucket_values_by_pieces / bucket_tail_by_pieces take, as k_moments_pieces: one
// lane per piece of 64 values, every lane decoding in every step, the cell of a run flushed at every bucket edge -
// entries [e0, e1) of the call (entry e at e - e0), one per bucket the piece's visible values reach. Timestamps are
// regular there: the time of every value, and so its x, is arithmetic.
__global__ __launch_bounds__(MDB_WAVE) void k_trend_pieces(DevSegments s, BucketRequest r, const uint32_t *__restrict__ groups,
                                                      const unsigned long long *__restrict__ piece_base,
                                                      const MvCursor *__restrict__ cursors, unsigned long long n_pieces,
                                                      const unsigned long long *__restrict__ offsets,
                                                      unsigned long long e0, unsigned long long e1,
                                                      unsigned long long *__restrict__ keys,
                                                      mdb_comoments_cell *__restrict__ out) {
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
    TrendRun run = trend_run_empty();
    uint64_t bucket = b_first;
    uint64_t bucket_base = trend_bucket_base(r.origin, r.width, b_first);
    auto flush = [&]() {
        const uint64_t e = base + (bucket - b_first);
        if (e >= e0 && e < e1) {
            keys[e - e0] = row + bucket;
            out[e - e0] = trend_finish(run);
        }
        run = trend_run_empty();
        bucket++;
        bucket_base += (uint64_t)r.width;
    };
    auto take = [&](uint32_t k, uint32_t bits) {
        if (k < to_skip || k >= to_decode) return;
        const int64_t t = start + (int64_t)((uint64_t)(point_index + k) * (uint64_t)delta);
        const uint64_t b = ((uint64_t)t - (uint64_t)r.origin) / (uint64_t)r.width;
        while (bucket < b) flush();
        trend_point(run, bucket_base, t, __uint_as_float(bits));
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

// The buckets of the device batch `in` (groups: a device array or nullptr) merged into a device array of n_cells
// cells. `host_cells` (host forms): the caller's array, which is uploaded, merged into and downloaded instead; either
// way nothing of the caller's is written unless the whole call succeeds.
static int trend_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_bucket_request *request,
                     uint64_t n_cells, mdb_comoments_cell *dev_cells, mdb_comoments_cell *host_cells) {
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
    // The MacaqueV streams of the batch's cursor index (MDB_GRID_MV_INDEX=0: none) go piece by piece: their entries
    // are folded behind the pairs, in slices of their own.
    std::shared_ptr<MvIndex> index;
    const unsigned long long *piece_base = nullptr, *entry_offsets = nullptr;
    unsigned long long entries = 0;
    if (mv_index_for_range(ctx, in, &index, &piece_base)) return 1;
    if (piece_base && bucket_pieces_count(ctx, s, r, piece_base, *index, &entry_offsets, &entries)) return 1;

    const uint64_t slice = slice_pairs_setting();
    const uint64_t pair_slices = (total + slice - 1) / slice, entry_slices = (entries + slice - 1) / slice;
    const uint64_t n_slices = pair_slices + entry_slices;
    const uint64_t cap = std::min<uint64_t>(slice, std::max<uint64_t>(total, entries));
    BucketCells<mdb_comoments_cell> cells;
    if (cells.stage(ctx, n_cells, dev_cells, host_cells, n_slices)) return 1;
    BucketFold<ComomentsFoldOps> fold;
    if (fold.reserve(ctx, cap, n_cells)) return 1;
    mdb_comoments_cell *partials = fold.partials();
    unsigned long long *keys = fold.keys();

    for (uint64_t k = 0; k < n_slices; k++) {
        // (slices of pairs first, then slices of the pieces' entries)
        const bool pairs = k < pair_slices;
        const uint64_t p0 = (pairs ? k : k - pair_slices) * slice;
        const uint64_t p1 = std::min<uint64_t>(p0 + slice, pairs ? total : entries), m = p1 - p0;
        MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
        if (pairs) {
            LaunchTimer timer(ctx, "k_trend_partials");
            hipLaunchKernelGGL(k_trend_partials, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, r,
                               offsets, p0, p1, partials, keys, words, piece_base);
        } else {
            const uint64_t n_pieces = index->n_pieces;
            LaunchTimer timer(ctx, "k_trend_pieces");
            hipLaunchKernelGGL(k_trend_pieces, dim3((uint32_t)((n_pieces + MDB_WAVE - 1) / MDB_WAVE)), dim3(MDB_WAVE), 0,
                               ctx->stream, s, r, groups, piece_base, static_cast<const MvCursor *>(index->cursors),
                               (unsigned long long)n_pieces, entry_offsets, p0, p1, keys, partials);
        }
        unsigned int error = 0;
        bool unsorted = false;
        if (bucket_slice_check(ctx, keys, m, words, &error, &unsorted)) return 1;
        if (error) return fail(describe_error(error));
        if (fold.fold_slice(ctx, m, unsorted, cells.cells())) return 1;
    }
    return cells.commit();
}

int trend_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                   uint32_t n_inputs, const mdb_bucket_request *request, uint64_t n_cells, mdb_comoments_cell *inout) {
    // (an upload the library holds, as mdb_moments_buckets_list: the batch gets the cursor index a resident batch gets)
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, false)) return 1;
    return trend_run(ctx, list.segments(), list.groups(), request, n_cells, nullptr, inout);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_trend_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                                     const mdb_bucket_request *request, mdb_comoments_cell *inout) {
    if (!ctx || !in || !request || !inout) return fail("ctx, in, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (trend_request_check(request, &n_cells)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return trend_run(ctx, in, group_of_segment, request, n_cells, inout, nullptr);
}
