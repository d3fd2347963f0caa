// mdb_m4.hip - M4 downsampling on segments (mdb_m4_buckets*): per date_bin bucket and group the first, last, lowest
// and highest point with their timestamps, and the count - no point materialised.
//
// What the reference answers with GridExec -> AggregateExec(first_value / last_value ORDER BY ts, min, max) and a join
// back onto the points for the timestamps of the extremes. The structure is that of mdb_buckets.hip, whose span, scan,
// key check and sort are shared (mdb_buckets.hpp), as are the reduction tree and the fold - one template for every
// per-bucket operator (mdb_bucket_fold.hpp, M4FoldOps below); the partial carries four points instead of four numbers:
//
//   k_agg_bucket_span   (shared) the buckets each segment reaches, its group id checked; a scan makes pair offsets.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS pairs, slices folded one after the other:
//   k_m4_partials       1 lane / segment with pairs in the slice: the record and the cell key of each pair. PMC-Mean on
//                       regular timestamps: O(1). Swing on regular timestamps: O(log n), exact - the ends, and one
//                       binary search for the earliest point that already has the far end's value (m4_model_points).
//                       Residual tails, MacaqueV values, irregular timestamps: decoded once (m4_stream_partials).
//                       Streams in the batch's cursor index are left to
//   k_m4_pieces         1 lane / piece of 64 values, one entry {key, record} per bucket the piece reaches; the entries
//                       are reduced and folded like the pairs, in slices behind them.
//   k_agg_bucket_check  (shared) keys non-decreasing? If not, a stable radix sort by key.
//   k_m4_tree           (k_bucket_tree<M4FoldOps>) runs of equal keys reduced through a fixed tree of 64-entry tiles.
//   k_m4_fold           (k_bucket_fold<M4FoldOps>) 1 lane / pair: the lane of a run's last pair folds the run and merges
//                       it into the cell. No two lanes write one cell, no atomics on cells.
// The four rules are minima under total orders (mdb_m4.hpp), so the bytes of a cell do not depend on the order in
// which anything above happens.
//
// Scratch layout: a partial is a 64-byte RECORD, mdb_m4_cell's 56 bytes padded, 64-byte aligned, read and written as
// four 16-byte words - not split arrays: a lane writes the records of ITS segment's pairs one after the other, so
// the words of one record are what lies together in memory, and a record is one 64-byte sector. With the 8-byte key:
// 72 B per pair written and read back (mdb_agg_buckets: 24 + 8).
#include "mdb_bucket_fold.hpp"
#include "mdb_m4.hpp"
#include "mdb_scan.hpp"

#include <algorithm>

namespace mdb {

// What the tree and fold (mdb_bucket_fold.hpp) need to know of a record: its four 16-byte words, the four rules.
struct M4FoldOps : FoldOps<M4Partial, mdb_m4_cell> {
    static constexpr const char *tree_name = "k_m4_tree", *fold_name = "k_m4_fold";
    __device__ __forceinline__ static M4Partial load(const M4Partial *from) { return m4_load(from); }
    __device__ __forceinline__ static void store(M4Partial *to, const M4Partial &value) { m4_store(to, value); }
    __device__ __forceinline__ static M4Partial empty() { return m4_empty(); }
    __device__ __forceinline__ static void merge(M4Partial &into, const M4Partial &from) { m4_merge(into, from); }
    __device__ __forceinline__ static bool is_empty(const M4Partial &acc) { return acc.count == 0; }
    __device__ __forceinline__ void apply(mdb_m4_cell &cell, const M4Partial &acc) const { m4_merge(cell, acc); }
};

__global__ __launch_bounds__(BUCKET_THREADS) void k_m4_partials(DevSegments s, const uint32_t *__restrict__ groups,
                                                                BucketRequest r,
                                                                const unsigned long long *__restrict__ offsets,
                                                                uint64_t p0, uint64_t p1, M4Partial *__restrict__ out,
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
        // (an error: the call fails; by pieces: every point is k_m4_pieces' - the pairs stay empty)
        for (uint64_t j = j0; j < j1; j++) m4_store(&out[j - p0], m4_empty());
    } else {
        const bool tail_by_pieces = bucket_tail_by_pieces(s, i, info, piece_base); // (the model's points only, then)
        const bool regular = (info.desc.flags & FLAG_REGULAR) != 0;
        const bool stream = !regular || (info.desc.flags & FLAG_TYPE_MASK) == MDB_MACAQUE_V_ID;
        if (!stream) {
            for (uint64_t j = j0; j < j1; j++) {
                int64_t lo, hi;
                bucket_bounds(r, b_first + (j - off), &lo, &hi);
                M4Partial acc = m4_empty();
                m4_regular_pair(s, i, info, lo, hi, acc, &error, tail_by_pieces);
                m4_store(&out[j - p0], acc);
            }
        } else if (!m4_stream_partials(s, i, info, r, off, b_first, j0, j1, p0, out, &error)) {
            for (uint64_t j = j0; j < j1; j++) {
                int64_t lo, hi;
                bucket_bounds(r, b_first + (j - off), &lo, &hi);
                m4_unsorted_pair(s, i, info, lo, hi, j, p0, out, &error);
            }
        }
    }
    if (error) atomicOr(error_out, error);
}

// The pieces of the MacaqueV streams bucket_values_by_pieces / bucket_tail_by_pieces take, as k_agg_bucket_pieces
// (mdb_buckets.hip): one lane per piece of 64 values, every lane decoding in every step, a record flushed at every
// bucket edge - entries [e0, e1) of the call (entry e at e - e0), one per bucket the piece's visible values reach.
// Timestamps are regular there: the time of every value is known where it is decoded.
__global__ __launch_bounds__(MDB_WAVE) void k_m4_pieces(DevSegments s, BucketRequest r, const uint32_t *__restrict__ groups,
                                                        const unsigned long long *__restrict__ piece_base,
                                                        const MvCursor *__restrict__ cursors, unsigned long long n_pieces,
                                                        const unsigned long long *__restrict__ offsets,
                                                        unsigned long long e0, unsigned long long e1,
                                                        unsigned long long *__restrict__ keys,
                                                        M4Partial *__restrict__ out) {
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
    M4Partial acc = m4_empty();
    uint64_t bucket = b_first;
    auto flush = [&]() {
        const uint64_t e = base + (bucket - b_first);
        if (e >= e0 && e < e1) {
            keys[e - e0] = row + bucket;
            m4_store(&out[e - e0], acc);
        }
        acc = m4_empty();
        bucket++;
    };
    auto take = [&](uint32_t k, uint32_t bits) {
        if (k < to_skip || k >= to_decode) return;
        const int64_t t = start + (int64_t)((uint64_t)(point_index + k) * (uint64_t)delta);
        const uint64_t b = ((uint64_t)t - (uint64_t)r.origin) / (uint64_t)r.width;
        while (bucket < b) flush();
        m4_point(acc, t, __uint_as_float(bits));
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
static int m4_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_bucket_request *request,
                  uint64_t n_cells, mdb_m4_cell *dev_cells, mdb_m4_cell *host_cells) {
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
    BucketCells<mdb_m4_cell> cells;
    if (cells.stage(ctx, n_cells, dev_cells, host_cells, n_slices)) return 1;
    BucketFold<M4FoldOps> fold;
    if (fold.reserve(ctx, cap, n_cells)) return 1;
    M4Partial *partials = fold.partials();
    unsigned long long *keys = fold.keys();

    for (uint64_t k = 0; k < n_slices; k++) {
        // (slices of pairs first, then slices of the pieces' entries)
        const bool pairs = k < pair_slices;
        const uint64_t p0 = (pairs ? k : k - pair_slices) * slice;
        const uint64_t p1 = std::min<uint64_t>(p0 + slice, pairs ? total : entries), m = p1 - p0;
        MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
        if (pairs) {
            LaunchTimer timer(ctx, "k_m4_partials");
            hipLaunchKernelGGL(k_m4_partials, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, r,
                               offsets, p0, p1, partials, keys, words, piece_base);
        } else {
            const uint64_t n_pieces = index->n_pieces;
            LaunchTimer timer(ctx, "k_m4_pieces");
            hipLaunchKernelGGL(k_m4_pieces, dim3((uint32_t)((n_pieces + MDB_WAVE - 1) / MDB_WAVE)), dim3(MDB_WAVE), 0,
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

int m4_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                uint32_t n_inputs, const mdb_bucket_request *request, uint64_t n_cells, mdb_m4_cell *inout) {
    // (an upload the library holds, as mdb_agg_buckets_list: the batch gets the cursor index a resident batch gets)
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, false)) return 1;
    return m4_run(ctx, list.segments(), list.groups(), request, n_cells, nullptr, inout);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_m4_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                                  const mdb_bucket_request *request, mdb_m4_cell *inout) {
    if (!ctx || !in || !request || !inout) return fail("ctx, in, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (m4_request_check(request, &n_cells)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return m4_run(ctx, in, group_of_segment, request, n_cells, inout, nullptr);
}
