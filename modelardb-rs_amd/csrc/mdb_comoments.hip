// mdb_comoments.hip - covariance and correlation of two fields on segments (mdb_comoments_buckets*): per date_bin
// bucket and group the count, both means, both m2 and c_xy = the sum of (x - mean_x) * (y - mean_y).
//
// What the reference answers with GridExec per field -> SortedJoinExec -> AggregateExec(corr / covar_samp / covar_pop /
// regr_*): its model-based rule rewrites only count / min / max / sum / avg, so every point of both fields is rebuilt
// and zipped by row position (query/sorted_join_exec.rs:278-310). Here the x field is walked on its segments with the
// structure of mdb_moments.hip, and the y field is the row masks' construction (mdb_mask.hip) with one f32 per row in
// place of one bit:
//
//   rows and first rows    the range grid's prepass of x under [t_lo, t_hi] (grid_range_plan: every error the range
//                          calls report) and an exclusive scan give each x segment its first row; the prepass of y
//                          gives its row count. The two counts must agree: row r of x is then row r of y however
//                          differently the fields were cut into segments.
//   the y column           the range grid of y, values only (no timestamp is written), into ycol[n_rows] in scratch:
//                          4 B per row, in HBM only - the one thing the operator materialises.
//   k_agg_bucket_span      (shared) the buckets each x segment reaches, its group id checked; a scan makes pair offsets.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS pairs, slices folded one after the other:
//   k_comoments_partials   1 lane / x segment with pairs in the slice: the cell and the cell key of each pair. PMC-Mean
//                          and Swing on regular timestamps: point by point in registers, ycol[row] read per point (no
//                          O(1) case: the y side needs every row). Residual tails, MacaqueV values, irregular
//                          timestamps: decoded once (comoments_stream_partials). Streams in the batch's cursor index
//                          are left to
//   k_comoments_pieces     1 lane / piece of 64 values, one entry {key, cell} per bucket the piece reaches; the entries
//                          are reduced and folded like the pairs, in slices behind them.
//   k_agg_bucket_check     (shared) keys non-decreasing? If not, a stable radix sort by key.
//   k_comoments_tree       (k_bucket_tree<ComomentsFoldOps>) runs of equal keys reduced through a fixed tree of 64-entry
//                          tiles.
//   k_comoments_fold       (k_bucket_fold<ComomentsFoldOps>) 1 lane / pair: the lane of a run's last pair folds the run
//                          and merges it into the cell. No two lanes write one cell, no atomics on cells.
// The tree and the fold are the one template of every per-bucket operator (mdb_bucket_fold.hpp), instantiated with
// ComomentsFoldOps (mdb_comoments.hpp).
// The row of a point is its segment's first row plus the number of the segment's earlier points inside [t_lo, t_hi]:
// what segment_range (mdb_agg_dev.hpp) calls the row of a point and the mask consumers test a bit at.
// Every run is summed around its first pair (mdb_comoments.hpp) and runs meet only in comoments_merge, in an order fixed
// by the input, the request and the slice size: two runs of a call agree bit for bit, and a different order of merges
// moves the f64 members by rounding only. All stores are ordinary vector stores.
//
// Scratch: 48 B per pair (the cell) and the 8-byte key, 4 B per row of y, 12 B per segment of x for the row plan.
#include "mdb_comoments.hpp"
#include "mdb_scan.hpp"

#include <algorithm>
#include <string>

namespace mdb {

__global__ __launch_bounds__(BUCKET_THREADS) void k_comoments_partials(
    DevSegments s, const uint32_t *__restrict__ groups, BucketRequest r, const unsigned long long *__restrict__ offsets,
    uint64_t p0, uint64_t p1, mdb_comoments_cell *__restrict__ out, unsigned long long *__restrict__ keys,
    unsigned int *__restrict__ error_out, const unsigned long long *__restrict__ piece_base,
    const unsigned long long *__restrict__ first_row, YColumn y) {
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
        // (an error: the call fails; by pieces: every point is k_comoments_pieces' - the pairs stay empty)
        for (uint64_t j = j0; j < j1; j++) out[j - p0] = comoments_empty();
    } else {
        const bool tail_by_pieces = bucket_tail_by_pieces(s, i, info, piece_base); // (the model's points only, then)
        const bool regular = (info.desc.flags & FLAG_REGULAR) != 0;
        const bool stream = !regular || (info.desc.flags & FLAG_TYPE_MASK) == MDB_MACAQUE_V_ID;
        const uint64_t segment_row = first_row[i];
        if (!stream) {
            const SegDesc &d = info.desc;
            uint32_t k_first = 0, k_last = 0; // the segment's points inside [t_lo, t_hi]: point k_first is its row 0
            (void)regular_index_interval(d.start, d.delta, d.n_total, r.t_lo, r.t_hi, &k_first, &k_last);
            for (uint64_t j = j0; j < j1; j++) {
                int64_t lo, hi;
                bucket_bounds(r, b_first + (j - off), &lo, &hi);
                out[j - p0] = comoments_regular_pair(s, i, info, lo, hi, segment_row - k_first, y, &error, tail_by_pieces);
            }
        } else if (!comoments_stream_partials(s, i, info, r, off, b_first, j0, j1, p0, out, segment_row, y, &error)) {
            for (uint64_t j = j0; j < j1; j++) {
                int64_t lo, hi;
                bucket_bounds(r, b_first + (j - off), &lo, &hi);
                comoments_unsorted_pair(s, i, info, r, lo, hi, j, p0, out, segment_row, y, &error);
            }
        }
    }
    if (error) atomicOr(error_out, error);
}

// The pieces of the MacaqueV streams bucket_values_by_pieces / bucket_tail_by_pieces take, as k_moments_pieces: one
// lane per piece of 64 values, every lane decoding in every step, the cell of a run flushed at every bucket edge -
// entries [e0, e1) of the call (entry e at e - e0), one per bucket the piece's visible values reach. Timestamps are
// regular there: the time and the row of every value are known where it is decoded.
__global__ __launch_bounds__(MDB_WAVE) void k_comoments_pieces(
    DevSegments s, BucketRequest r, const uint32_t *__restrict__ groups, const unsigned long long *__restrict__ piece_base,
    const MvCursor *__restrict__ cursors, unsigned long long n_pieces, const unsigned long long *__restrict__ offsets,
    unsigned long long e0, unsigned long long e1, unsigned long long *__restrict__ keys,
    mdb_comoments_cell *__restrict__ out, const unsigned long long *__restrict__ first_row, YColumn y,
    unsigned int *__restrict__ error_out) {
    __shared__ uint32_t ring[PIECE_RING_ROWS][MDB_WAVE];
    const int lane = threadIdx.x;
    const unsigned long long piece = (unsigned long long)blockIdx.x * MDB_WAVE + lane;
    const uint8_t *values_first = first_buffer(s.values), *residuals_first = first_buffer(s.residuals); // (see view_data())
    uint32_t to_decode = 0, to_skip = 0, point_index = 0;
    uint64_t b_first = 0, b_last = 0, base = 0, row = 0, row_base = 0;
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
            uint32_t k_first = 0, k_last = 0; // the segment's points inside [t_lo, t_hi]: point k_first is its row 0
            (void)regular_index_interval(info.desc.start, info.desc.delta, info.desc.n_total, r.t_lo, r.t_hi, &k_first, &k_last);
            row_base = first_row[cursor.segment()] - k_first + point_index;
            piece_open(reader, s, cursor, values_first, residuals_first);
            state = piece_state(cursor, seed);
        }
    }
    if (!__any(to_decode > 0)) return;
    ComomentsRun run = comoments_run_empty();
    uint32_t error = 0;
    uint64_t bucket = b_first;
    auto flush = [&]() {
        const uint64_t e = base + (bucket - b_first);
        if (e >= e0 && e < e1) {
            keys[e - e0] = row + bucket;
            out[e - e0] = comoments_finish(run);
        }
        run = comoments_run_empty();
        bucket++;
    };
    auto take = [&](uint32_t k, uint32_t bits) {
        if (k < to_skip || k >= to_decode) return;
        const int64_t t = start + (int64_t)((uint64_t)(point_index + k) * (uint64_t)delta);
        const uint64_t b = ((uint64_t)t - (uint64_t)r.origin) / (uint64_t)r.width;
        while (bucket < b) flush();
        comoments_point(run, __uint_as_float(bits), y.at(row_base + k, &error));
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
    if (error) atomicOr(error_out, error);
}

// The rows of x and y under [t_lo, t_hi] compared, x's first rows (n + 1, in SCRATCH_COMOMENTS_ROWS: a slot of its
// own, the range grid of y and the row masks use theirs meanwhile) and the y column (SCRATCH_COMOMENTS_YCOL).
int comoments_rows(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, int64_t t_lo, int64_t t_hi,
                   const unsigned long long **first_row, YColumn *column) {
    const uint64_t n = x->n;
    if (n > 0xffffffffull) return fail("Too many segments for one call of mdb_comoments_buckets*.");
    const uint64_t b4 = align_up(n * 4, 256), b8 = align_up((n + 1) * 8, 256);
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_COMOMENTS_ROWS, b4 + b8 + align_up(scan_block_sums_bytes(n), 256), &p)) return 1;
    Carver scratch(p);
    unsigned long long *first = scratch.take<unsigned long long>(n + 1);
    unsigned long long *block_sums = scratch.take<unsigned long long>(scan_block_sums_bytes(n) / 8);
    uint32_t *rows = scratch.take<uint32_t>(n);
    uint64_t x_rows = 0, y_rows = 0;
    if (grid_range_plan(ctx, x, t_lo, t_hi, &x_rows, nullptr, rows)) return 1;
    if (device_exclusive_scan(ctx, ItemsOf<uint32_t>{rows}, n, first, block_sums, "k_comoments_scan")) return 1;
    if (y != x && grid_range_plan(ctx, y, t_lo, t_hi, &y_rows, nullptr, nullptr)) return 1;
    if (y == x) y_rows = x_rows;
    if (x_rows != y_rows)
        return fail("The x field has " + std::to_string(x_rows) + " rows under the time range but the y field has " +
                    std::to_string(y_rows) + " rows: the batches do not line up.");
    const uint64_t bytes = x_rows * 4;
    if (ctx->scratch_limit && bytes > ctx->scratch_limit)
        return fail("The y column of " + std::to_string(x_rows) + " rows needs " + std::to_string(bytes) +
                    " bytes of scratch but the context's limit is " + std::to_string(ctx->scratch_limit) +
                    ": cut the batch by series.");
    if (scratch_reserve(ctx, SCRATCH_COMOMENTS_YCOL, bytes, &p)) return 1;
    float *values = static_cast<float *>(p);
    uint64_t written = 0;
    if (grid_batch_dev_locked(ctx, y, TimeRange{t_lo, t_hi, 1}, nullptr, values, nullptr, x_rows, &written, nullptr)) return 1;
    if (written != x_rows) return fail("The range grid of the y field changed its row count between two passes.");
    *first_row = first;
    *column = YColumn{values, x_rows};
    return 0;
}

// The buckets of the device batches x and y (groups: a device array or nullptr) merged into a device array of n_cells
// cells. `host_cells` (host forms): the caller's array, which is uploaded, merged into and downloaded instead; either
// way nothing of the caller's is written unless the whole call succeeds.
static int comoments_run(mdb_ctx *ctx, const mdb_segments *in, const mdb_segments *y_in, const uint32_t *groups,
                         const mdb_bucket_request *request, uint64_t n_cells, mdb_comoments_cell *dev_cells,
                         mdb_comoments_cell *host_cells) {
    const uint64_t n = in->n;
    if (n == 0 || request->n_buckets == 0) return 0;
    const BucketRequest r = {request->origin, request->width, request->n_buckets, request->t_lo, request->t_hi,
                             request->n_groups, request->which_mask};
    if (n > UINT64_MAX / request->n_buckets)
        return fail("Too many (segment, bucket) pairs for one call: split the batch.");
    const unsigned long long *first_row = nullptr;
    YColumn y{nullptr, 0};
    if (comoments_rows(ctx, in, y_in, r.t_lo, r.t_hi, &first_row, &y)) return 1;
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
            LaunchTimer timer(ctx, "k_comoments_partials");
            hipLaunchKernelGGL(k_comoments_partials, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, r,
                               offsets, p0, p1, partials, keys, words, piece_base, first_row, y);
        } else {
            const uint64_t n_pieces = index->n_pieces;
            LaunchTimer timer(ctx, "k_comoments_pieces");
            hipLaunchKernelGGL(k_comoments_pieces, dim3((uint32_t)((n_pieces + MDB_WAVE - 1) / MDB_WAVE)), dim3(MDB_WAVE), 0,
                               ctx->stream, s, r, groups, piece_base, static_cast<const MvCursor *>(index->cursors),
                               (unsigned long long)n_pieces, entry_offsets, p0, p1, keys, partials, first_row, y,
                               words);
        }
        unsigned int error = 0;
        bool unsorted = false;
        if (bucket_slice_check(ctx, keys, m, words, &error, &unsorted)) return 1;
        if (error & ERR_COMOMENTS_ROW)
            return fail("(internal) A row of the x field lies beyond the y column: the row plan and the range grid "
                        "disagree.");
        if (error) return fail(describe_error(error));
        if (fold.fold_slice(ctx, m, unsorted, cells.cells())) return 1;
    }
    return cells.commit();
}

int comoments_list_run(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                       uint32_t n_y, const uint32_t *const *group_of_segment_x, const mdb_bucket_request *request,
                       uint64_t n_cells, mdb_comoments_cell *inout) {
    // (uploads the library holds, as mdb_moments_buckets_list: the batches get the cursor index a resident batch gets)
    UploadedSegments lists(ctx);
    if (lists.upload_pair(xs, n_x, ys, n_y, group_of_segment_x)) return 1;
    return comoments_run(ctx, lists.segments(), lists.y_segments(), lists.groups(), request, n_cells, nullptr, inout);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_comoments_buckets_dev(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y,
                                         const uint32_t *group_of_segment_x, const mdb_bucket_request *request,
                                         mdb_comoments_cell *inout) {
    if (!ctx || !x || !y || !request || !inout) return fail("ctx, x, y, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (comoments_request_check(request, &n_cells)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return comoments_run(ctx, x, y, group_of_segment_x, request, n_cells, inout, nullptr);
}
