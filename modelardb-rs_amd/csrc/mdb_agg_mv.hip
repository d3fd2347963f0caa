// mdb_agg_mv.hip - aggregates over MacaqueV value streams, as a service to mdb_agg.hip.
//   mv_index_stream_sums   SUM from a cursor index into the streams (MvIndex), a lane per piece of 64 values
//                          (mdb_mv_pieces.hpp): k_agg_mv_pieces, then k_agg_mv_chain_groups for streams of several pieces.
//   mv_index_range_totals  SUM / COUNT / MIN / MAX under a time range from the same cursors: k_agg_mv_range.
//   macaque_deferred       without cursors, the long streams k_agg_segments / k_agg_range leave aside: decoded into
//                          scratch by mv_pipeline (mdb_mv_parallel.hip) or by a lane per stream, k_mv_sums / k_mv_range_*.
#include "mdb_agg_dev.hpp"
#include "mdb_segment_dev.hpp"
#include "mdb_scan.hpp"
#include "mdb_macaque_parallel.hpp"
#include "mdb_mv_pieces.hpp"

namespace mdb {

// ---- the same cursors for SUM: macaque_v::sum adds a stream's values one after the other in f32 --------------
//
// f32 addition does not associate, so the additions of one stream stay a chain - but 64 chains fit into a wave, and
// the decoding, a hundred times the work, is again one lane per piece: k_agg_mv_pieces decodes every piece of the
// batch into scratch (piece p at values[64 p ..]: a stream's values follow each other), with the seeds sum() uses
// (models/mod.rs:145-181: the model's last DECODED value, NaN behind a MacaqueV model), and k_agg_mv_chains adds
// every stream up with one lane. stream_sums[2 i] = the sum of MacaqueV segment i's values (macaque_v.rs:228-235:
// it starts AS the first value), [2 i + 1] = the sum of segment i's residual tail.
struct ChainItem { // 16 bytes: a stream of two pieces or more, listed by the wave of k_agg_mv_pieces it begins in
    uint32_t segment_and_kind; // segment << 1 | 1 for its residual tail
    uint32_t n;                // its values, if it ends in the wave it begins in (0: it goes on - its segment's analysis knows)
    unsigned long long first_piece;
};

// Is piece `piece` (of segment i's values or of its tail) the first / the last of its stream? (The pieces of a stream
// follow each other in the cursor index.)
__device__ __forceinline__ void piece_neighbours(const MvCursor *__restrict__ cursors, unsigned long long piece, unsigned long long n_pieces,
                                                 uint32_t i, bool residual, bool *is_head, bool *is_tail) {
    if (piece == 0) {
        *is_head = true;
    } else {
        const MvCursor *before = cursors + piece - 1;
        *is_head = load_global(&before->segment) != i || ((load_global(&before->window) & MV_WINDOW_RESIDUAL) != 0) != residual;
    }
    if (piece + 1 == n_pieces) {
        *is_tail = true;
    } else {
        const MvCursor *behind = cursors + piece + 1;
        *is_tail = load_global(&behind->segment) != i || ((load_global(&behind->window) & MV_WINDOW_RESIDUAL) != 0) != residual;
    }
}

// Which lanes of a wave of pieces list a stream - the first pieces of streams of two pieces or more -, of which kind
// (short: up to CHAIN_SHORT_VALUES values; long: more, or going on behind the wave, where only the segment's analysis
// knows how many), with how many values, and the lane's place among the wave's listed streams of its kind.
constexpr uint32_t CHAIN_SHORT_VALUES = 1024;
struct ChainListing {
    bool lists, is_long;
    uint32_t n;                // values of the stream; 0: it goes on behind the wave
    uint32_t rank;             // among the wave's listed streams of the same kind
    uint32_t n_short, n_long;  // of the wave
};
__device__ __forceinline__ ChainListing chain_listing(bool present, bool is_head, bool is_tail, uint32_t to_decode, int lane) {
    ChainListing out;
    out.lists = present && is_head && !is_tail;
    const unsigned long long tails = __ballot(present && is_tail);
    const unsigned long long tails_behind = lane == 63 ? 0ull : (tails >> (lane + 1));
    const int my_tail = tails_behind ? lane + 1 + __builtin_ctzll(tails_behind) : -1; // (none: the stream goes on behind the wave)
    const uint32_t last_count = (uint32_t)__shfl((int)to_decode, my_tail >= 0 ? my_tail : lane, MDB_WAVE);
    out.n = my_tail >= 0 ? (uint32_t)(my_tail - lane) * MV_PIECE_VALUES + last_count : 0u; // (64 a piece but the last)
    out.is_long = out.n == 0u || out.n > CHAIN_SHORT_VALUES;
    const unsigned long long shorts = __ballot(out.lists && !out.is_long), longs = __ballot(out.lists && out.is_long);
    const unsigned long long below = (1ull << lane) - 1ull;
    out.rank = (uint32_t)__popcll((out.is_long ? longs : shorts) & below);
    out.n_short = (uint32_t)__popcll(shorts);
    out.n_long = (uint32_t)__popcll(longs);
    return out;
}

// How many streams of either kind every wave of pieces lists: long << 32 | short (the scan over these says where).
__global__ __launch_bounds__(MDB_WAVE) void k_agg_mv_chain_count(const MvCursor *__restrict__ cursors, unsigned long long n_pieces,
                                                                 unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x;
    const unsigned long long piece = (unsigned long long)blockIdx.x * MDB_WAVE + lane;
    bool is_head = false, is_tail = false;
    uint32_t to_decode = 0;
    if (piece < n_pieces) {
        const PieceCursor cursor = load_piece_cursor(cursors, piece);
        to_decode = cursor.n_values();
        piece_neighbours(cursors, piece, n_pieces, cursor.segment(), cursor.residual(), &is_head, &is_tail);
    }
    const ChainListing listing = chain_listing(piece < n_pieces, is_head, is_tail, to_decode, lane);
    if (lane == 0) counts[blockIdx.x] = ((unsigned long long)listing.n_long << 32) | listing.n_short;
}

// One lane per piece, as k_grid_mv_pieces (the same decoder, rounds of ROUND values staged in LDS): a piece that is a
// whole stream - most residual tails are - is added up by its own lane while it is decoded (its values ARE the stream,
// in order); the pieces of longer streams go to `values` (piece p at 64 p, rows of ROUND consecutive values per store)
// and the stream is listed for k_agg_mv_chain_groups by the lane of its first piece. (Round 5's kernel staged all 64
// values of every piece - 22 KB of LDS a wave, 1.75 waves a SIMD - so that the lane of a stream's first piece could add
// up the stream inside the wave while the other 63 waited: 2.7 / 2.3 ms where this decoder needs 2.0 / 1.45 for grid().)
template <int ROUND>
__global__ __launch_bounds__(MDB_WAVE) void k_agg_mv_pieces(DevSegments s, const MvCursor *__restrict__ cursors,
                                                            unsigned long long n_pieces, uint32_t *__restrict__ values,
                                                            float *__restrict__ stream_sums, ChainItem *__restrict__ short_items,
                                                            ChainItem *__restrict__ long_items,
                                                            const unsigned long long *__restrict__ chain_offsets) {
    constexpr int STRIDE = ROUND + 1; // (a row per lane: an odd stride keeps the banks apart)
    __shared__ uint32_t stage[MDB_WAVE * STRIDE];
    __shared__ uint32_t ring[PIECE_RING_ROWS][MDB_WAVE];
    __shared__ uint32_t row_count[MDB_WAVE];
    const int lane = threadIdx.x;
    const unsigned long long first_piece = (unsigned long long)blockIdx.x * MDB_WAVE;
    const unsigned long long piece = first_piece + lane;
    const uint8_t *values_first = first_buffer(s.values), *residuals_first = first_buffer(s.residuals); // (see view_data())
    uint32_t to_decode = 0, segment = 0xffffffffu;
    bool residual = false, is_head = false, is_tail = false;
    PieceReader reader;
    PieceState state = piece_state_idle();
    reader.idle(cursors);
    if (piece < n_pieces) {
        const PieceCursor cursor = load_piece_cursor(cursors, piece);
        const uint32_t i = cursor.segment();
        segment = i;
        to_decode = cursor.n_values();
        residual = cursor.residual();
        piece_neighbours(cursors, piece, n_pieces, i, residual, &is_head, &is_tail);
        piece_open(reader, s, cursor, values_first, residuals_first);
        // (the seed of sum(), models/mod.rs:145-181: the model's last DECODED value, NaN behind a MacaqueV model)
        uint32_t seed = 0;
        if (residual) {
            const int32_t type = s.model_type_id[i];
            if (type == MDB_PMC_MEAN_ID) {
                float value = 0.0f;
                (void)decode_pmc_value(s.values.views[i], s.min_value[i], s.max_value[i], &value);
                seed = __float_as_uint(value);
            } else if (type == MDB_SWING_ID) {
                float first = 0.0f, last = 0.0f;
                (void)decode_swing_values(s.values.views[i], s.min_value[i], s.max_value[i], &first, &last);
                seed = __float_as_uint(last);
            } else {
                seed = 0x7fc00000u; // f32::NAN (models/mod.rs:167)
            }
        }
        state = piece_state(cursor, seed);
    }
    const bool present = piece < n_pieces;
    const bool whole = present && is_head && is_tail; // the piece is its stream: summed here
    const bool spilled = present && !whole;           // a piece of a longer stream: its values go to memory
    // The streams of two pieces or more that begin in this wave, listed where the scan says (k_agg_mv_chain_count made
    // the same tests): the short ones in one list, the long ones in another.
    {
        const ChainListing listing = chain_listing(present, is_head, is_tail, to_decode, lane);
        if (listing.lists) {
            const unsigned long long where = chain_offsets[blockIdx.x];
            ChainItem *to = listing.is_long ? long_items + (where >> 32) : short_items + (where & 0xffffffffull);
            to[listing.rank] = {(segment << 1) | (residual ? 1u : 0u), listing.n, piece};
        }
    }
    piece_start(reader, ring, lane);
    // macaque_v.rs:220-265: a segment's values are added to the first one, a tail's to 0, one after the other.
    float own = 0.0f;
    const bool starts_as_first = !residual;
    for (uint32_t done = 0; __any(done < to_decode); done += ROUND) {
        const uint32_t mine = done < to_decode ? min(to_decode - done, (uint32_t)ROUND) : 0u;
        static_assert(ROUND % 2 == 0, "values are decoded in pairs");
        for (uint32_t k = 0, most = wave_max_u32(mine); k < most; k += 2) {
            if (__any(reader.hungry())) reader.top_up(ring, lane);
            const uint32_t even = piece_decode_value(reader, state, ring, lane);
            const uint32_t odd = piece_decode_value(reader, state, ring, lane);
            stage[lane * STRIDE + k] = even;
            stage[lane * STRIDE + k + 1] = odd; // (k + 1 == ROUND: the row's spare word)
            // (the running sum of the lane's own piece: what a piece that is a whole stream reports)
            const float with_even = (starts_as_first && done + k == 0u) ? __uint_as_float(even) : own + __uint_as_float(even);
            own = k < mine ? with_even : own;
            own = k + 1 < mine ? own + __uint_as_float(odd) : own;
        }
        // Row r = this round's values of lane r's piece, for the pieces that go to memory: consecutive values,
        // (64 / ROUND) rows per store instruction.
        row_count[lane] = spilled ? mine : 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        constexpr int ROWS_PER_STORE = MDB_WAVE / ROUND;
        const int sub_row = lane / ROUND, column_of_lane = lane % ROUND;
        constexpr int BATCH = 8;
        static_assert(MDB_WAVE % (BATCH * ROWS_PER_STORE) == 0, "whole batches of stores");
        for (int r0 = 0; r0 < MDB_WAVE; r0 += BATCH * ROWS_PER_STORE) {
            uint32_t counts[BATCH], staged[BATCH];
#pragma unroll
            for (int q = 0; q < BATCH; q++) {
                const int r = r0 + q * ROWS_PER_STORE + sub_row;
                counts[q] = row_count[r];
                staged[q] = stage[r * STRIDE + column_of_lane];
            }
#pragma unroll
            for (int q = 0; q < BATCH; q++) {
                const int r = r0 + q * ROWS_PER_STORE + sub_row;
                if ((uint32_t)column_of_lane < counts[q])
                    values[(first_piece + (unsigned long long)r) * MV_PIECE_VALUES + done + (uint32_t)column_of_lane] = staged[q];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (whole && to_decode > 0) stream_sums[2ull * segment + (residual ? 1u : 0u)] = own;
}

// A stream of two pieces or more: its values lie in `values` (piece p at 64 p), and its f32 additions are one chain,
// in stream order (macaque_v.rs:228-235). A chain is 4 cycles an addition; what it waited for was memory - a lane of
// its own kept 128 bytes of its stream in flight, a round trip per 32 additions (round 6's counters: 65 % of the
// kernel's wave-cycles waiting, the vector ALU busy 5 %; a 65 536-value stream 0.7 ms) - and, in front of that, a thread
// per SEGMENT that looked for the streams not summed yet (0.75 ms for 8.5 M segments). Now the waves of k_agg_mv_pieces
// list the streams that begin in them (k_agg_mv_chain_count + a scan say where), and k_agg_mv_chain_groups gives every
// listed stream EIGHT lanes: together they keep 2 KB of it in flight - a round of 512 values, 16 chunks of 16 bytes per
// lane, the eight lanes' chunks side by side in memory - park a round in LDS, ask for the next one, and the first of
// the eight adds the parked round up, value after value.
// Two sizes of round: most listed streams are a few pieces long (a stretch of rejected points between two models) and
// want many waves in flight more than bytes - 4 loads a lane, 128 values a round, 4 KB of LDS a wave; the long ones
// (a whole chunk of noise is one stream of 65 536 values) want the bytes - 16 loads a lane, 512 values a round. A list
// of its own for each kind (a stream that goes on behind its wave counts as long): the long chains begin at once
// instead of behind the dispatch of the short ones' hundred thousand waves.
constexpr int CHAIN_GROUP_LANES = 8;
constexpr int CHAIN_GROUPS_PER_WAVE = MDB_WAVE / CHAIN_GROUP_LANES;

// Cursors left by host threads (the index of one call): should they ever disagree with the kernels' own analysis about
// a segment's streams, its sums are made unusable rather than a little wrong. (A resident batch's cursors come from
// that same analysis, k_mv_index_walk: nothing to compare.)
__global__ __launch_bounds__(256) void k_agg_mv_check_cursors(DevSegments s, const uint32_t *__restrict__ known_totals,
                                                              const unsigned long long *__restrict__ piece_base,
                                                              float *__restrict__ stream_sums) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    const unsigned long long first_piece = piece_base[i];
    if (piece_base[i + 1] == first_piece) return; // (no stream: nobody reads this segment's sums)
    uint32_t n_values, n_res, n_model, error;
    mv_stream_lengths(s, i, known_totals, &n_values, &n_res, &n_model, &error);
    if ((unsigned long long)((n_values + MV_PIECE_VALUES - 1) / MV_PIECE_VALUES + (n_res + MV_PIECE_VALUES - 1) / MV_PIECE_VALUES) !=
        piece_base[i + 1] - first_piece)
        stream_sums[2 * i] = stream_sums[2 * i + 1] = __uint_as_float(0x7fc00000u);
}

template <int CHAIN_LOADS> // 16-byte loads a lane has in flight: 4 for the list of short streams, 16 for the long ones
__global__ __launch_bounds__(MDB_WAVE) void k_agg_mv_chain_groups(DevSegments s, const uint32_t *__restrict__ known_totals,
                                                                  const uint32_t *__restrict__ values, float *__restrict__ stream_sums,
                                                                  const ChainItem *__restrict__ items, unsigned int n_items) {
    constexpr int CHAIN_ROUND_CHUNKS = CHAIN_LOADS * CHAIN_GROUP_LANES; // chunks of 16 bytes = 4 values a round
    constexpr int CHAIN_GROUP_STRIDE = CHAIN_ROUND_CHUNKS + 1;          // (in chunks: the eight adding lanes read eight banks)
    __shared__ uint4 parked[CHAIN_GROUPS_PER_WAVE * CHAIN_GROUP_STRIDE];
    const int lane = threadIdx.x, group = lane / CHAIN_GROUP_LANES, member = lane % CHAIN_GROUP_LANES;
    const unsigned int mine = blockIdx.x * CHAIN_GROUPS_PER_WAVE + (unsigned int)group;
    const bool listed = mine < n_items;
    ChainItem item{0u, 1u, 0ull}; // (a group without a stream: one value of the scratch's first piece, nobody's sum)
    if (listed) item = items[mine];
    // How many values the stream has: its pieces said so if it ended in the wave it began in, else the analysis of
    // its segment, by the group's first lane.
    uint32_t n = item.n;
    const bool tail = (item.segment_and_kind & 1u) != 0u;
    if (listed && member == 0 && n == 0) {
        uint32_t n_values, n_res, n_model, error;
        mv_stream_lengths(s, item.segment_and_kind >> 1, known_totals, &n_values, &n_res, &n_model, &error);
        n = tail ? n_res : n_values;
    }
    n = (uint32_t)__shfl((int)n, group * CHAIN_GROUP_LANES, MDB_WAVE);
    const uint32_t n_chunks = (n + 3u) >> 2;
    const uint4 *__restrict__ from = reinterpret_cast<const uint4 *>(values + item.first_piece * MV_PIECE_VALUES);
    uint4 *mine_parked = parked + group * CHAIN_GROUP_STRIDE;
    auto ask = [&](uint32_t round, uint4 (&into)[CHAIN_LOADS]) { // chunk j * 8 + member of the round: the group's lanes side by side
#pragma unroll
        for (int j = 0; j < CHAIN_LOADS; j++) {
            const uint32_t chunk = round * CHAIN_ROUND_CHUNKS + (uint32_t)(j * CHAIN_GROUP_LANES + member);
            into[j] = chunk < n_chunks ? load_global(from + chunk) : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    const uint32_t rounds = (n_chunks + CHAIN_ROUND_CHUNKS - 1) / CHAIN_ROUND_CHUNKS;
    const uint32_t most_rounds = wave_max_u32(rounds);
    // macaque_v.rs:228-235: the sum of a MacaqueV segment's values starts AS the first of them, a tail's at zero.
    const bool starts_as_first = !tail;
    float sum = 0.0f;
    uint4 asked[CHAIN_LOADS];
    ask(0, asked);
    for (uint32_t round = 0; round < most_rounds; round++) {
#pragma unroll
        for (int j = 0; j < CHAIN_LOADS; j++) mine_parked[j * CHAIN_GROUP_LANES + member] = asked[j];
        wave_sync();
        if (round + 1 < most_rounds) ask(round + 1, asked); // (under way while the round that is parked is added up)
        if (member == 0 && round < rounds) {
            const uint32_t first_value = round * (uint32_t)(4 * CHAIN_ROUND_CHUNKS);
            const uint32_t here = min(n - first_value, (uint32_t)(4 * CHAIN_ROUND_CHUNKS)); // values of this round
            uint32_t k = 0;
            if (round == 0 && starts_as_first) {
                const uint4 q = mine_parked[0];
                sum = __uint_as_float(q.x);
                if (here > 1) sum += __uint_as_float(q.y);
                if (here > 2) sum += __uint_as_float(q.z);
                if (here > 3) sum += __uint_as_float(q.w);
                k = 4;
            }
            for (; k + 32 <= here; k += 32) { // (eight reads of the parked round under way, then the chain of additions;
                                              // the next batch's reads under way during the additions: slower, 0.77 -> 0.92 ms)
                uint4 q[8];
#pragma unroll
                for (int j = 0; j < 8; j++) q[j] = mine_parked[(k >> 2) + (uint32_t)j];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    sum += __uint_as_float(q[j].x);
                    sum += __uint_as_float(q[j].y);
                    sum += __uint_as_float(q[j].z);
                    sum += __uint_as_float(q[j].w);
                }
            }
            for (; k + 4 <= here; k += 4) {
                const uint4 q = mine_parked[k >> 2];
                sum += __uint_as_float(q.x);
                sum += __uint_as_float(q.y);
                sum += __uint_as_float(q.z);
                sum += __uint_as_float(q.w);
            }
            if (k < here) { // (the stream's last, partial chunk)
                const uint4 q = mine_parked[k >> 2];
                sum += __uint_as_float(q.x);
                if (k + 1 < here) sum += __uint_as_float(q.y);
                if (k + 2 < here) sum += __uint_as_float(q.z);
            }
        }
        wave_sync(); // (the next round overwrites what was parked)
    }
    if (member == 0 && listed && n > 0) stream_sums[2ull * (item.segment_and_kind >> 1) + (tail ? 1u : 0u)] = sum;
}

// The f32 sums of all MacaqueV streams of a batch that has a cursor index (see k_agg_mv_pieces);
// *stream_sums stays nullptr when it has none. known_totals: of the caller's own counting walk (may be nullptr).
int mv_index_stream_sums(mdb_ctx *ctx, const mdb_segments *in, const DevSegments &s, const uint32_t *known_totals,
                         const float **stream_sums, const unsigned long long **only_with_pieces) {
    *stream_sums = nullptr;
    *only_with_pieces = nullptr;
    std::shared_ptr<MvIndex> index = mv_index_lookup(in);
    if (!index) return 0;
    {
        std::lock_guard<std::mutex> lock(index->mutex);
        if (!index->built || !index->usable) return 0; // (built by the first grid call, or by agg_run before its own walk)
    }
    // (the index of one call covers its long streams only: the sums of a segment without pieces are nobody's)
    if (index->of_one_call) *only_with_pieces = static_cast<const unsigned long long *>(index->piece_base);
    const uint64_t piece_waves = (index->n_pieces + MDB_WAVE - 1) / MDB_WAVE;
    if (piece_waves > 0x7ffffff0ull) return fail("Too many MacaqueV streams for one batch.");
    // (every listed stream has two pieces or more)
    const uint64_t most_items = index->n_pieces / 2 + 1;
    const uint64_t counts_bytes = align_up(piece_waves * 8, 256), offsets_bytes = align_up((piece_waves + 1) * 8, 256);
    const uint64_t block_sums_bytes = align_up(scan_block_sums_bytes(piece_waves), 256);
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_AGG_MV, index->n_pieces * MV_PIECE_VALUES * 4 + in->n * 8 + 256, &p)) return 1;
    uint32_t *values = static_cast<uint32_t *>(p);
    float *sums = reinterpret_cast<float *>(values + index->n_pieces * MV_PIECE_VALUES);
    // (a stream without values - the tail of a segment that has none - sums to 0: the kernels write the others)
    MDB_HIP_CHECK(hipMemsetAsync(sums, 0, 8 * in->n, ctx->stream));
    void *q = nullptr;
    if (scratch_reserve(ctx, SCRATCH_AGG_CHAIN_LIST, counts_bytes + offsets_bytes + block_sums_bytes + 2 * most_items * sizeof(ChainItem) + 64, &q)) return 1;
    uint8_t *at = static_cast<uint8_t *>(q);
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(at);
    unsigned long long *offsets = reinterpret_cast<unsigned long long *>(at + counts_bytes);
    unsigned long long *block_sums = reinterpret_cast<unsigned long long *>(at + counts_bytes + offsets_bytes);
    ChainItem *short_items = reinterpret_cast<ChainItem *>(at + counts_bytes + offsets_bytes + block_sums_bytes);
    ChainItem *long_items = short_items + most_items;
    const MvCursor *cursors = static_cast<const MvCursor *>(index->cursors);
    // Where every wave of pieces lists the streams of two pieces or more that begin in it: a function of the cursors
    // alone, so the index of a resident batch keeps it from the first call that asks (MDB_AGG_KEEP_CHAIN_OFFSETS=0:
    // counted by every call, as the index of one call over host batches is).
    unsigned long long listed = 0;
    bool counted_before = false;
    const char *keep_setting = option_text("MDB_AGG_KEEP_CHAIN_OFFSETS");
    const bool keep = !index->of_one_call && !(keep_setting && std::strcmp(keep_setting, "0") == 0);
    if (keep) {
        std::lock_guard<std::mutex> lock(index->mutex);
        if (index->chains_built) {
            offsets = static_cast<unsigned long long *>(index->chain_offsets);
            listed = index->chains_listed;
            counted_before = true;
        }
    }
    if (!counted_before) {
        void *kept = nullptr;
        if (keep && hipMalloc(&kept, (piece_waves + 1) * 8) != hipSuccess) { // (no memory to keep it in: counted every time)
            (void)hipGetLastError();
            kept = nullptr;
        }
        if (kept) offsets = static_cast<unsigned long long *>(kept);
        {
            LaunchTimer timer(ctx, "k_agg_mv_chain_count");
            hipLaunchKernelGGL(k_agg_mv_chain_count, dim3((uint32_t)piece_waves), dim3(MDB_WAVE), 0, ctx->stream, cursors, index->n_pieces, counts);
        }
        int failed = device_exclusive_scan(ctx, ItemsOf<unsigned long long>{counts}, piece_waves, offsets, block_sums, "k_agg_mv_chain_scan");
        // (how many are listed sizes the launches behind the piece kernel: a wave that finds nothing to do still costs a
        // third of a microsecond, and the most there can be is 5.4 M groups for the mixed series' 10.8 M pieces)
        if (!failed && (mail_read(ctx, &listed, offsets + piece_waves, 8) != hipSuccess || mail_sync(ctx) != hipSuccess))
            failed = fail("Could not read how many MacaqueV streams the pieces list.");
        if (failed) {
            if (kept) (void)hipFree(kept);
            return 1;
        }
        if (kept) { // (complete: the stream has been waited for) - unless another context's call has left its own meanwhile
            std::lock_guard<std::mutex> lock(index->mutex);
            if (!index->chains_built) {
                index->chain_offsets = kept;
                index->chains_listed = listed;
                index->chains_built = true;
                kept = nullptr;
            } else {
                offsets = static_cast<unsigned long long *>(index->chain_offsets);
            }
        }
        if (kept) MDB_HIP_CHECK(hipFree(kept));
    }
    const uint64_t n_short = listed & 0xffffffffull, n_long = listed >> 32;
    if (n_short > most_items || n_long > most_items) return fail("Internal error: more MacaqueV streams listed than there are pieces for.");
    {
        LaunchTimer timer(ctx, "k_agg_mv_pieces");
        hipLaunchKernelGGL(k_agg_mv_pieces<32>, dim3((uint32_t)piece_waves), dim3(MDB_WAVE), 0, ctx->stream, s, cursors, index->n_pieces,
                           values, sums, short_items, long_items, static_cast<const unsigned long long *>(offsets));
    }
    {
        // The listed streams, eight lanes each: the long kind first (they are what takes longest), the short kind behind.
        LaunchTimer timer(ctx, "k_agg_mv_chains");
        if (n_long > 0)
            hipLaunchKernelGGL((k_agg_mv_chain_groups<16>), dim3((uint32_t)((n_long + CHAIN_GROUPS_PER_WAVE - 1) / CHAIN_GROUPS_PER_WAVE)),
                               dim3(MDB_WAVE), 0, ctx->stream, s, known_totals, values, sums, long_items, (unsigned int)n_long);
        if (n_short > 0)
            hipLaunchKernelGGL((k_agg_mv_chain_groups<4>), dim3((uint32_t)((n_short + CHAIN_GROUPS_PER_WAVE - 1) / CHAIN_GROUPS_PER_WAVE)),
                               dim3(MDB_WAVE), 0, ctx->stream, s, known_totals, values, sums, short_items, (unsigned int)n_short);
        if (index->of_one_call)
            hipLaunchKernelGGL(k_agg_mv_check_cursors, dim3((uint32_t)((in->n + 255) / 256)), dim3(256), 0, ctx->stream, s, known_totals,
                               static_cast<const unsigned long long *>(index->piece_base), sums);
    }
    *stream_sums = sums;
    return 0;
}

// ---- SUM over long MacaqueV streams --------------------------------------------------------------------
//
// macaque_v::sum (macaque_v.rs:220-265) adds the values of a stream one after the other in f32, and
// f32 addition does not associate, so the additions stay with one lane per stream. What need not stay
// there is the decoding, which is a hundred times the work: k_agg_segments leaves the streams that
// qualify for the parallel decoder aside, they are decoded into scratch memory here, and k_mv_sums
// then only has to add floats.

constexpr unsigned long long DEFERRED_ONE = 1ull << 40; // scan item: streams above bit 40, their values below

struct DeferredItem {
    DevSegments s;
    uint32_t min_values;
    TimeRange range;
    const unsigned long long *by_pieces; // (under a time range: the index whose segments k_agg_mv_range takes, or nullptr)
    __device__ uint64_t operator()(uint64_t i) const {
        if (s.model_type_id[i] != MDB_MACAQUE_V_ID) return 0;
        const SegInfo info = analyse_segment(s, i);
        if (by_pieces && by_pieces[i + 1] > by_pieces[i] && mv_range_by_pieces(s, i, info)) return 0;
        const uint32_t values = mv_deferred_values(s, i, info, min_values, range);
        return values ? (DEFERRED_ONE | values) : 0;
    }
};

__global__ __launch_bounds__(256) void k_mv_select_scanned(DevSegments s, TimeRange range,
                                                           const unsigned long long *__restrict__ scan,
                                                           uint32_t min_values, MvSeg *__restrict__ segs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    const unsigned long long mine = scan[i];
    if ((scan[i + 1] >> 40) == (mine >> 40)) return; // not one of the streams left aside
    SegInfo info = analyse_segment(s, i);
    if (range.enabled) apply_time_range(s, i, info, range);
    segs[mine >> 40] = mv_describe(s, i, info, min_values, mine & (DEFERRED_ONE - 1));
}

struct DeferredResult {
    double sum;
    long long count; // the three below: time-range aggregates only
    float min;
    float max;
    unsigned int error;
    unsigned int pad;
};

// One wave per stream. The additions are a dependent chain that only one lane can walk, so the wave's
// job is to keep that lane fed: all lanes fetch the next MV_SUM_CHUNK values (coalesced, in flight
// while lane 0 adds up the chunk before) and hand them over through LDS.
constexpr uint32_t MV_SUM_CHUNK = 1024;

__global__ __launch_bounds__(MDB_WAVE) void k_mv_sums(const MvSeg *__restrict__ segs, uint64_t n_slots,
                                                      const float *__restrict__ values, float *__restrict__ sums,
                                                      DeferredResult *__restrict__ result) {
    __shared__ float4 chunk_lds[2][MV_SUM_CHUNK / 4];
    const uint32_t slot = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const MvSeg seg = segs[slot];
    if (!seg.done) {
        // The parallel decoder gave this stream up: decode it here, one lane.
        if (lane != 0) return;
        float sum = 0.0f;
        uint32_t error = 0;
        decode_macaque_v(reinterpret_cast<const uint8_t *>(seg.words) + seg.bias_bits / 8, seg.total_bits / 8,
                         seg.n_model, false, 0, &error, [&](uint32_t k, uint32_t bits) {
                             if (k == 0) sum = __uint_as_float(bits);
                             else sum += __uint_as_float(bits);
                         });
        if (error) atomicOr(&result->error, error);
        sums[slot] = sum;
        return;
    }
    constexpr uint32_t PER_LANE = MV_SUM_CHUNK / MDB_WAVE;
    const float *__restrict__ v = values + seg.out_offset;
    const uint32_t n = seg.n_model;
    float fetched[PER_LANE];
    auto fetch = [&](uint32_t base) {
#pragma unroll
        for (uint32_t j = 0; j < PER_LANE; j++) {
            const uint32_t k = base + j * MDB_WAVE + lane;
            fetched[j] = k < n ? v[k] : 0.0f;
        }
    };
    auto hand_over = [&](uint32_t buffer) {
        float *to = reinterpret_cast<float *>(chunk_lds[buffer]);
#pragma unroll
        for (uint32_t j = 0; j < PER_LANE; j++) to[j * MDB_WAVE + lane] = fetched[j];
    };
    fetch(0);
    hand_over(0);
    __syncthreads();
    float sum = 0.0f;
    uint32_t buffer = 0;
    for (uint32_t base = 0; base < n; base += MV_SUM_CHUNK, buffer ^= 1u) {
        const bool more = base + MV_SUM_CHUNK < n;
        if (more) fetch(base + MV_SUM_CHUNK);
        if (lane == 0) {
            const uint32_t count = min(MV_SUM_CHUNK, n - base);
            const float4 *from = chunk_lds[buffer];
            uint32_t k = 0;
            if (base == 0) { // the sum starts AS the first value (macaque_v.rs:228-235)
                const float *first = reinterpret_cast<const float *>(from);
                sum = first[0];
                for (k = 1; k < 4 && k < count; k++) sum += first[k];
            }
#pragma unroll 4
            for (; k + 4 <= count; k += 4) {
                const float4 q = from[k / 4];
                sum += q.x;
                sum += q.y;
                sum += q.z;
                sum += q.w;
            }
            const float *rest = reinterpret_cast<const float *>(from);
            for (; k < count; k++) sum += rest[k];
        }
        if (more) hand_over(buffer ^ 1u);
        __syncthreads();
    }
    if (lane == 0) sums[slot] = sum;
}

// The same sums when there are too many streams for the parallel decoder to pay off: one lane per
// stream decodes (LDS ring, as k_grid_serial) and adds as it goes.
__global__ __launch_bounds__(SERIAL_THREADS) void k_mv_serial_sums(const MvSeg *__restrict__ segs, uint64_t n_slots,
                                                                  float *__restrict__ sums,
                                                                  DeferredResult *__restrict__ result) {
    __shared__ uint32_t ring[SERIAL_RING_WORDS][MDB_WAVE];
    const int lane = threadIdx.x;
    const uint64_t slot = (uint64_t)blockIdx.x * SERIAL_THREADS + lane;
    bool active = slot < n_slots;
    RingBitReader reader;
    reader.begin(nullptr, 0);
    MacaqueStream stream;
    stream.remaining = 0; stream.position = 0; stream.last = 0;
    stream.leading = 255; stream.trailing = 0; stream.first_is_raw = true; stream.fresh = true;
    if (active) {
        const MvSeg seg = segs[slot];
        reader.begin(reinterpret_cast<const uint8_t *>(seg.words) + seg.bias_bits / 8, seg.total_bits / 8);
        stream.remaining = seg.n_model;
        active = seg.n_model > 0 && seg.total_bits > 0;
    }
    float sum = 0.0f;
    uint32_t error = 0;
    while (__any(active)) {
        if (__any(active && reader.hungry())) ring_top_up(reader, ring, lane, active);
        if (active) {
            const bool first = stream.first_is_raw;
            bool malformed;
            const float value = __uint_as_float(ring_decode_value(reader, stream, ring, lane, &malformed));
            sum = first ? value : sum + value; // the sum starts AS the first value (macaque_v.rs:228-235)
            stream.remaining -= 1;
            // A stream shorter than its segment claims ends the loop too: it is bounded by the bits
            // there are, not by a (possibly corrupted) count.
            if (malformed || reader.overrun()) error |= ERR_BITSTREAM;
            if (malformed || reader.overrun() || stream.remaining == 0) active = false;
        }
    }
    if (slot < n_slots) sums[slot] = sum;
    if (error) atomicOr(&result->error, error);
}

constexpr int MV_FINISH_THREADS = 1024;

// ---- the same for aggregates under a time range: SUM (f64), COUNT, MIN, MAX of the visible values ----------

__device__ __forceinline__ RangeAcc shfl_down_partial(const RangeAcc &p, int delta) {
    RangeAcc q;
    const unsigned long long sum_bits = (unsigned long long)__double_as_longlong(p.sum);
    q.sum = __longlong_as_double((long long)(((unsigned long long)__shfl_down((uint32_t)(sum_bits >> 32), delta, MDB_WAVE) << 32) |
                                             __shfl_down((uint32_t)sum_bits, delta, MDB_WAVE)));
    q.count = (long long)(((unsigned long long)__shfl_down((uint32_t)((unsigned long long)p.count >> 32), delta, MDB_WAVE) << 32) |
                          __shfl_down((uint32_t)p.count, delta, MDB_WAVE));
    q.min = __shfl_down(p.min, delta, MDB_WAVE);
    q.max = __shfl_down(p.max, delta, MDB_WAVE);
    return q;
}

// One wave per stream the parallel decoder has put into `values` (its visible values only).
__global__ __launch_bounds__(MDB_WAVE) void k_mv_range_partials(const MvSeg *__restrict__ segs, uint64_t n_slots,
                                                                const float *__restrict__ values,
                                                                RangeAcc *__restrict__ partials,
                                                                DeferredResult *__restrict__ result) {
    const uint32_t slot = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const MvSeg seg = segs[slot];
    RangeAcc mine;
    if (!seg.done) {
        // The parallel decoder gave this stream up: decode it here, one lane.
        if (lane != 0) return;
        uint32_t error = 0;
        decode_macaque_v(reinterpret_cast<const uint8_t *>(seg.words) + seg.bias_bits / 8, seg.total_bits / 8,
                         seg.visible_end, false, 0, &error, [&](uint32_t k, uint32_t bits) {
                             if (k >= seg.first) mine.point(__uint_as_float(bits));
                         });
        if (error) atomicOr(&result->error, error);
        partials[slot] = mine;
        return;
    }
    const float *__restrict__ v = values + seg.out_offset;
    const uint32_t n = seg.visible_end - seg.first;
    for (uint32_t k = lane; k < n; k += MDB_WAVE) mine.point(v[k]);
#pragma unroll
    for (int delta = MDB_WAVE / 2; delta > 0; delta >>= 1) mine.merge(shfl_down_partial(mine, delta));
    if (lane == 0) partials[slot] = mine;
}

// One lane per stream, out of the LDS ring (too many streams for the parallel decoder to pay off).
__global__ __launch_bounds__(SERIAL_THREADS) void k_mv_serial_range(const MvSeg *__restrict__ segs, uint64_t n_slots,
                                                                   RangeAcc *__restrict__ partials,
                                                                   DeferredResult *__restrict__ result) {
    __shared__ uint32_t ring[SERIAL_RING_WORDS][MDB_WAVE];
    const int lane = threadIdx.x;
    const uint64_t slot = (uint64_t)blockIdx.x * SERIAL_THREADS + lane;
    bool active = slot < n_slots;
    RingBitReader reader;
    reader.begin(nullptr, 0);
    MacaqueStream stream;
    stream.remaining = 0; stream.position = 0; stream.last = 0;
    stream.leading = 255; stream.trailing = 0; stream.first_is_raw = true; stream.fresh = true;
    uint32_t first = 0;
    if (active) {
        const MvSeg seg = segs[slot];
        reader.begin(reinterpret_cast<const uint8_t *>(seg.words) + seg.bias_bits / 8, seg.total_bits / 8);
        stream.remaining = seg.visible_end; // the format has no random access: from the beginning
        first = seg.first;
        active = seg.visible_end > 0 && seg.total_bits > 0;
    }
    RangeAcc mine;
    uint32_t error = 0;
    while (__any(active)) {
        if (__any(active && reader.hungry())) ring_top_up(reader, ring, lane, active);
        if (active) {
            bool malformed;
            const float value = __uint_as_float(ring_decode_value(reader, stream, ring, lane, &malformed));
            if (stream.position >= first) mine.point(value);
            stream.position += 1;
            stream.remaining -= 1;
            if (malformed || reader.overrun()) error |= ERR_BITSTREAM;
            if (malformed || reader.overrun() || stream.remaining == 0) active = false;
        }
    }
    if (slot < n_slots) partials[slot] = mine;
    if (error) atomicOr(&result->error, error);
}

__global__ __launch_bounds__(MV_FINISH_THREADS) void k_mv_range_finish(const RangeAcc *__restrict__ partials,
                                                                       uint64_t n_slots,
                                                                       DeferredResult *__restrict__ result) {
    // (a type with default member initialisers cannot be declared __shared__: its storage can)
    __shared__ double lds_storage[MV_FINISH_THREADS * sizeof(RangeAcc) / sizeof(double)];
    RangeAcc *lds = reinterpret_cast<RangeAcc *>(lds_storage);
    RangeAcc mine;
    for (uint64_t slot = threadIdx.x; slot < n_slots; slot += MV_FINISH_THREADS) mine.merge(partials[slot]);
    lds[threadIdx.x] = mine;
    __syncthreads();
    for (int width = MV_FINISH_THREADS / 2; width > 0; width >>= 1) {
        if ((int)threadIdx.x < width) {
            RangeAcc a = lds[threadIdx.x];
            a.merge(lds[threadIdx.x + width]);
            lds[threadIdx.x] = a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        result->sum = lds[0].sum;
        result->count = lds[0].count;
        result->min = lds[0].min;
        result->max = lds[0].max;
    }
}

// Aggregates under a time range over a batch with cursors into its MacaqueV streams (a resident batch's sidecar, or
// what the call's host threads left): one lane per piece of 64 values, as k_grid_mv_pieces - but only the pieces that
// reach into the range are decoded, and only as far as it goes; what the points inside it contribute (GridExec +
// filter + aggregate: f64 sum of the f32 values, count, extremes) is reduced per wave. Taken are the MacaqueV
// segments with regular timestamps, no residuals and pieces in the index - the ones k_agg_range leaves out by the
// same test (mv_range_by_pieces) - and the residual tails of PMC-Mean and Swing segments with regular timestamps
// (mv_range_tail_by_pieces; a resident batch's index has their cursors: in k_agg_range a tenth of the lanes of a
// wave would each decode one while the others wait).
__global__ __launch_bounds__(MDB_WAVE) void k_agg_mv_range(DevSegments s, TimeRange range, const MvCursor *__restrict__ cursors,
                                                           unsigned long long n_pieces, RangeAcc *__restrict__ partials) {
    __shared__ uint32_t ring[PIECE_RING_ROWS][MDB_WAVE];
    const int lane = threadIdx.x;
    const unsigned long long piece = (unsigned long long)blockIdx.x * MDB_WAVE + lane;
    const uint8_t *values_first = first_buffer(s.values), *residuals_first = first_buffer(s.residuals); // (see view_data())
    RangeAcc mine;
    uint32_t to_decode = 0, to_skip = 0;
    PieceReader reader;
    PieceState state = piece_state_idle();
    reader.idle(cursors);
    if (piece < n_pieces) {
        const PieceCursor cursor = load_piece_cursor(cursors, piece);
        const uint32_t i = cursor.segment(), point_index = cursor.point_index(), n_values = cursor.n_values();
        // (a segment with irregular timestamps is not this kernel's, mv_range_by_pieces: it is left before the analysis,
        // which would walk its timestamp stream to count its points - 0.9 ms per 10^9 points of such series)
        const uint4 ts_view = s.timestamps.views[i];
        const bool irregular = (int32_t)ts_view.x > 0 && (view_inline_byte(ts_view, 0) & 0x80u) != 0;
        if (!irregular && !(s.end_time[i] < range.lo || s.start_time[i] > range.hi)) {
            SegInfo info = analyse_segment(s, i);
            const bool residual = cursor.residual();
            if (residual ? mv_range_tail_by_pieces(s, i, info) : mv_range_by_pieces(s, i, info)) {
                // (a tail is XOR-seeded with the model's last RECONSTRUCTED value, models/mod.rs:241-249: what grid() sees)
                const uint32_t seed = residual ? __float_as_uint(info.desc.value) : 0u;
                apply_time_range(s, i, info, range);
                const uint32_t from = max(point_index, info.desc.first);
                const uint32_t upto = min(point_index + n_values, info.desc.first + info.desc.n_visible);
                if (info.desc.n_visible > 0 && from < upto) {
                    to_decode = upto - point_index;
                    to_skip = from - point_index;
                    piece_open(reader, s, cursor, values_first, residuals_first);
                    state = piece_state(cursor, seed);
                }
            }
        }
    }
    if (!__any(to_decode > 0)) { // (no piece of the wave reaches into the range)
        if (lane == 0) partials[blockIdx.x] = mine;
        return;
    }
    piece_start(reader, ring, lane);
    // (every lane decodes in every step - straight-line code -, the values wanted are taken)
    for (uint32_t k = 0, most = wave_max_u32(to_decode); k < most; k += 2) {
        if (__any(reader.hungry())) reader.top_up(ring, lane);
        const uint32_t even = piece_decode_value(reader, state, ring, lane);
        const uint32_t odd = piece_decode_value(reader, state, ring, lane);
        if (k >= to_skip && k < to_decode) mine.point(__uint_as_float(even));
        if (k + 1 >= to_skip && k + 1 < to_decode) mine.point(__uint_as_float(odd));
    }
#pragma unroll
    for (int delta = MDB_WAVE / 2; delta > 0; delta >>= 1) mine.merge(shfl_down_partial(mine, delta));
    if (lane == 0) partials[blockIdx.x] = mine;
}

// One workgroup, fixed order (strided partial sums, then a fixed tree): the result does not depend
// on how the work was scheduled.
__global__ __launch_bounds__(MV_FINISH_THREADS) void k_mv_sums_finish(const float *__restrict__ sums, uint64_t n_slots,
                                                                      DeferredResult *__restrict__ result) {
    __shared__ double partial[MV_FINISH_THREADS];
    double sum = 0.0;
    for (uint64_t slot = threadIdx.x; slot < n_slots; slot += MV_FINISH_THREADS) sum += (double)sums[slot];
    partial[threadIdx.x] = sum;
    __syncthreads();
    for (int width = MV_FINISH_THREADS / 2; width > 0; width >>= 1) {
        if ((int)threadIdx.x < width) partial[threadIdx.x] += partial[threadIdx.x + width];
        __syncthreads();
    }
    if (threadIdx.x == 0) result->sum = partial[0];
}

// The long MacaqueV streams k_agg_segments / k_agg_range left aside (mv_deferred_values; the caller has
// counted them: n_streams streams, n_values values to decode into scratch memory at most, n_bytes
// bytes). Without a range: each stream added up in f32 in stream order, the streams in f64
// (totals->sum). With one: SUM (f64), COUNT, MIN and MAX of the values inside it. *handled stays
// false only when the counts are beyond what the scan item can carry.
int macaque_deferred(mdb_ctx *ctx, const DevSegments &s, TimeRange range, uint32_t min_values, bool forced,
                     uint64_t n_streams, uint64_t n_values, uint64_t n_bytes, bool *handled,
                     DeferredTotals *totals, const unsigned long long *by_pieces) {
    *handled = false;
    if (n_streams == 0 || n_values >= DEFERRED_ONE) return 0;
    // Few enough streams for the parallel decoder (the gate of mv_pipeline)? Then their values go to
    // scratch memory first; otherwise a lane per stream decodes and accumulates in one go.
    const bool parallel = n_bytes * 8 / MV_PIECE_BITS + n_streams + 1 <= MV_MAX_PIECES || forced;
    const uint64_t scan_bytes = align_up((s.n + 1) * 8, 256);
    const uint64_t block_sums_bytes = align_up(scan_block_sums_bytes(s.n), 256);
    const uint64_t values_bytes = parallel ? align_up(n_values * 4, 256) : 256;
    const uint64_t per_stream_bytes = align_up(n_streams * sizeof(RangeAcc), 256); // or one float each
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_AGG_MV, scan_bytes + block_sums_bytes + values_bytes + per_stream_bytes + 256, &p))
        return 1;
    uint8_t *at = static_cast<uint8_t *>(p);
    unsigned long long *scan = reinterpret_cast<unsigned long long *>(at);
    at += scan_bytes;
    unsigned long long *block_sums = reinterpret_cast<unsigned long long *>(at);
    at += block_sums_bytes;
    float *values = reinterpret_cast<float *>(at);
    at += values_bytes;
    float *sums = reinterpret_cast<float *>(at);
    RangeAcc *partials = reinterpret_cast<RangeAcc *>(at);
    at += per_stream_bytes;
    DeferredResult *result = reinterpret_cast<DeferredResult *>(at);
    MDB_HIP_CHECK(hipMemsetAsync(result, 0, sizeof(DeferredResult), ctx->stream));
    if (device_exclusive_scan(ctx, DeferredItem{s, min_values, range, by_pieces}, s.n, scan, block_sums, "k_mv_deferred_scan"))
        return 1;
    auto select = [&](MvSeg *segs) {
        LaunchTimer timer(ctx, "k_mv_select");
        hipLaunchKernelGGL(k_mv_select_scanned, dim3((uint32_t)((s.n + 255) / 256)), dim3(256), 0, ctx->stream, s,
                           range, scan, min_values, segs);
    };
    MvSeg *segs = nullptr;
    if (parallel && mv_pipeline(ctx, n_streams, n_bytes, forced, select, values, &result->error, &segs)) return 1;
    const bool decoded = segs != nullptr;
    if (!decoded) {
        void *q = nullptr;
        if (scratch_reserve(ctx, SCRATCH_MV, n_streams * sizeof(MvSeg), &q)) return 1;
        segs = static_cast<MvSeg *>(q);
        select(segs);
    }
    const uint32_t lane_blocks = (uint32_t)((n_streams + SERIAL_THREADS - 1) / SERIAL_THREADS);
    if (range.enabled) {
        if (decoded) {
            LaunchTimer timer(ctx, "k_mv_range_partials");
            hipLaunchKernelGGL(k_mv_range_partials, dim3((uint32_t)n_streams), dim3(MDB_WAVE), 0, ctx->stream, segs,
                               n_streams, values, partials, result);
        } else {
            LaunchTimer timer(ctx, "k_mv_serial_range");
            hipLaunchKernelGGL(k_mv_serial_range, dim3(lane_blocks), dim3(SERIAL_THREADS), 0, ctx->stream, segs,
                               n_streams, partials, result);
        }
        LaunchTimer timer(ctx, "k_mv_range_finish");
        hipLaunchKernelGGL(k_mv_range_finish, dim3(1), dim3(MV_FINISH_THREADS), 0, ctx->stream, partials, n_streams,
                           result);
    } else {
        if (decoded) {
            LaunchTimer timer(ctx, "k_mv_sums");
            hipLaunchKernelGGL(k_mv_sums, dim3((uint32_t)n_streams), dim3(MDB_WAVE), 0, ctx->stream, segs, n_streams,
                               values, sums, result);
        } else {
            LaunchTimer timer(ctx, "k_mv_serial_sums");
            hipLaunchKernelGGL(k_mv_serial_sums, dim3(lane_blocks), dim3(SERIAL_THREADS), 0, ctx->stream, segs,
                               n_streams, sums, result);
        }
        LaunchTimer timer(ctx, "k_mv_sums_finish");
        hipLaunchKernelGGL(k_mv_sums_finish, dim3(1), dim3(MV_FINISH_THREADS), 0, ctx->stream, sums, n_streams, result);
    }
    DeferredResult host;
    MDB_HIP_CHECK(hipMemcpyAsync(&host, result, sizeof(DeferredResult), hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (host.error) return fail(describe_error(host.error));
    *handled = true;
    *totals = DeferredTotals{host.sum, host.count, host.min, host.max};
    return 0;
}

// For agg_run under a time range, with the index mv_index_for_range (mdb_grid.hip) gave it: what the indexed MacaqueV
// segments' points inside the range add up to (k_agg_mv_range).
int mv_index_range_totals(mdb_ctx *ctx, const DevSegments &s, TimeRange range, const MvIndex &index, DeferredTotals *totals) {
    const uint32_t n_blocks = (uint32_t)((index.n_pieces + MDB_WAVE - 1) / MDB_WAVE);
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_AGG_MV, (uint64_t)n_blocks * sizeof(RangeAcc) + 256, &p)) return 1;
    RangeAcc *partials = static_cast<RangeAcc *>(p);
    DeferredResult *result = reinterpret_cast<DeferredResult *>(reinterpret_cast<uint8_t *>(p) + align_up((uint64_t)n_blocks * sizeof(RangeAcc), 256));
    MDB_HIP_CHECK(hipMemsetAsync(result, 0, sizeof(DeferredResult), ctx->stream));
    {
        LaunchTimer timer(ctx, "k_agg_mv_range");
        hipLaunchKernelGGL(k_agg_mv_range, dim3(n_blocks), dim3(MDB_WAVE), 0, ctx->stream, s, range,
                           static_cast<const MvCursor *>(index.cursors), index.n_pieces, partials);
    }
    {
        LaunchTimer timer(ctx, "k_mv_range_finish");
        hipLaunchKernelGGL(k_mv_range_finish, dim3(1), dim3(MV_FINISH_THREADS), 0, ctx->stream, partials, (uint64_t)n_blocks, result);
    }
    DeferredResult host;
    MDB_HIP_CHECK(hipMemcpyAsync(&host, result, sizeof(DeferredResult), hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    *totals = DeferredTotals{host.sum, host.count, host.min, host.max};
    return 0;
}

} // namespace mdb
