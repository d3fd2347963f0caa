// mdb_mv_pieces.hpp - decoding MacaqueV value streams in a wave, device code only: the LDS ring of the kernels that
// give a lane a whole stream (k_grid_serial, k_mv_index_walk, k_mv_serial_*), and the decoder of the kernels that give
// a lane one PIECE of 64 values from the batch's cursor index (MvCursor, mdb_host_side.hpp), with the set-up they share:
// k_grid_mv_pieces (mdb_grid.hip), k_agg_mv_pieces, k_agg_mv_range (mdb_agg_mv.hip), k_agg_bucket_pieces (mdb_buckets.hip).
#pragma once

#include "mdb_segment_dev.hpp"

namespace mdb {

// ---- a lane per stream: the serial kernels' ring ------------------------------------------------------
//
// One lane per segment that carries a serial dependency, one wave per workgroup (k_grid_serial and the kernels
// that walk like it). MacaqueV streams (a model's values and/or the residual tail) are decoded from an LDS ring: every lane keeps the
// next SERIAL_RING_WORDS 32-bit words of ITS bitstream in LDS ([slot][lane], bank-conflict free),
// and when any lane runs low the whole wave tops all rings up with independent predicated loads
// issued back to back - one memory latency per ~24 words instead of one per word. The decode itself
// stays sequential per stream: value i's position depends on every earlier value.

constexpr int SERIAL_RING_WORDS = 32;
constexpr int SERIAL_TOPUP_WORDS = 24;
constexpr int SERIAL_THREADS = MDB_WAVE;

struct RingBitReader {
    const uint32_t *words; // aligned base in global memory
    uint32_t n_words;
    uint32_t next_word; // next word to move from the ring into the bit buffer
    uint32_t loaded;    // words [next_word, loaded) are in the ring
    uint64_t buffer;    // MSB aligned
    int32_t available;
    uint32_t skip_bits; // slack bits in front of the first payload byte
    uint64_t used_bits;
    uint64_t total_bits;
    uint32_t ahead;     // refill(): ring word next_word, byte swapped

    __device__ __forceinline__ void begin(const uint8_t *bytes, uint64_t nbytes) {
        uintptr_t address = reinterpret_cast<uintptr_t>(bytes);
        uint32_t misalign = (uint32_t)(address & 3u);
        words = reinterpret_cast<const uint32_t *>(address - misalign);
        n_words = (uint32_t)((nbytes + misalign + 3u) >> 2);
        next_word = 0;
        loaded = 0;
        buffer = 0;
        available = 0;
        skip_bits = 8u * misalign;
        used_bits = 0;
        total_bits = nbytes * 8u;
        ahead = 0;
    }
    __device__ __forceinline__ bool hungry() const { return loaded < n_words && loaded - next_word < 3; }
    __device__ __forceinline__ void pull(const uint32_t (*ring)[MDB_WAVE], int lane) {
        while (available <= 32 && next_word < loaded) {
            uint32_t w = __builtin_bswap32(ring[next_word % SERIAL_RING_WORDS][lane]);
            next_word += 1;
            if (skip_bits) { // only the very first word can carry slack bytes
                buffer |= ((uint64_t)w << 32) << skip_bits;
                available += 32 - (int32_t)skip_bits;
                skip_bits = 0;
            } else {
                buffer |= (uint64_t)w << (32 - available);
                available += 32;
            }
        }
    }
    __device__ __forceinline__ uint32_t get(uint32_t count, const uint32_t (*ring)[MDB_WAVE], int lane) {
        if (count == 0) return 0;
        pull(ring, lane);
        uint32_t value = (uint32_t)(buffer >> (64u - count));
        buffer <<= count;
        available -= (int32_t)count;
        used_bits += count;
        return value;
    }
    // The same without branches (64 lanes that each stand somewhere else in a code execute both sides
    // of every branch anyway): at most one word, so a caller that needs up to 45 bits refills before
    // the control bits and again before the payload. Needs 0 <= available while words remain, which
    // holds from the second refill of a stream on (the first word may bring as few as 8 bits).
    // The word comes out of a register (`ahead` = ring word next_word, see look_ahead) so that no LDS
    // latency sits on the chain from one code to the next.
    __device__ __forceinline__ void refill(const uint32_t (*ring)[MDB_WAVE], int lane) {
        const bool want = available <= 32 && next_word < loaded;
        const uint64_t placed = (((uint64_t)ahead << 32) << skip_bits) >> (available & 63);
        buffer |= want ? placed : 0ull;
        available += want ? 32 - (int32_t)skip_bits : 0;
        skip_bits = want ? 0u : skip_bits;
        next_word += want ? 1u : 0u;
        look_ahead(ring, lane);
    }
    // Ring slot of next_word, read whether or not it has been filled yet: it is not used before it has
    // (refill() tests next_word < loaded), and a stream that starts calls this again after its first
    // top-up. A top-up never overwrites the slots [next_word, loaded).
    __device__ __forceinline__ void look_ahead(const uint32_t (*ring)[MDB_WAVE], int lane) {
        ahead = __builtin_bswap32(ring[next_word % SERIAL_RING_WORDS][lane]);
    }
    __device__ __forceinline__ void consume(uint32_t count) {
        buffer <<= count;
        available -= (int32_t)count;
        used_bits += count;
    }
    __device__ __forceinline__ bool overrun() const { return used_bits > total_bits; }
};

struct MacaqueStream {
    uint32_t remaining;  // values still to decode
    uint32_t position;   // index of the next value inside the whole segment
    uint32_t last;       // bits of the previous value
    uint32_t leading, trailing;
    bool first_is_raw;   // the next value is stored as 32 raw bits (macaque_v.rs:289-293)
    bool fresh;          // nothing has been read from the stream yet
};

// Tops the ring of every lane of the wave up at once (the caller has found a hungry lane): independent
// predicated loads first, then the LDS writes.
__device__ __forceinline__ void ring_top_up(RingBitReader &reader, uint32_t (*ring)[MDB_WAVE], int lane, bool active) {
    uint32_t fetched[SERIAL_TOPUP_WORDS];
    const uint32_t first = reader.loaded;
    const uint32_t room = active ? SERIAL_RING_WORDS - (reader.loaded - reader.next_word) : 0u;
#pragma unroll
    for (int k = 0; k < SERIAL_TOPUP_WORDS; k++) {
        const uint32_t index = first + k;
        fetched[k] = ((uint32_t)k < room && index < reader.n_words) ? load_global(reader.words + index) : 0u;
    }
#pragma unroll
    for (int k = 0; k < SERIAL_TOPUP_WORDS; k++) {
        const uint32_t index = first + k;
        if ((uint32_t)k < room && index < reader.n_words) ring[index % SERIAL_RING_WORDS][lane] = fetched[k];
    }
    reader.loaded = min(reader.n_words, first + min(room, (uint32_t)SERIAL_TOPUP_WORDS));
}

// One value (macaque_v.rs:297-322): `10` it repeats, `0` + the bits of the previous window, `11` + 5
// bits leading zeros + 6 bits length + the bits - at most 45 bits, of which the control bits come off
// the top of the 64-bit buffer after one refill and the payload after another. Every lane of the wave
// stands at a different kind of code, so the three cases are computed with selects rather than
// branched to. Returns the bits of the value (stream.last is updated); *malformed: the window is
// impossible, the value returned is the previous one and the caller stops.
__device__ __forceinline__ uint32_t ring_decode_value(RingBitReader &reader, MacaqueStream &stream,
                                                      const uint32_t (*ring)[MDB_WAVE], int lane, bool *malformed) {
    if (stream.fresh) {
        reader.look_ahead(ring, lane);
        reader.refill(ring, lane);
        stream.fresh = false;
    }
    reader.refill(ring, lane);
    const uint32_t top = (uint32_t)(reader.buffer >> 51); // 13 bits: c0 c1 lz[5] len[6]
    const bool raw = stream.first_is_raw;                 // 32 raw bits, no control bits
    const bool c0 = (top >> 12) != 0u, c1 = ((top >> 11) & 1u) != 0u;
    const bool opens = !raw && c0 && c1;
    const bool repeats = !raw && c0 && !c1;
    const uint32_t header_bits = raw ? 0u : (c0 ? (c1 ? 13u : 2u) : 1u);
    const uint32_t leading = opens ? ((top >> 6) & 31u) : stream.leading;
    const uint32_t trailing = opens ? 32u - (top & 63u) - leading : stream.trailing;
    uint32_t meaningful = 32u - leading - trailing;
    *malformed = !raw && !repeats && (meaningful > 32u || trailing > 31u);
    const bool silent = repeats || *malformed; // no payload: the value is the previous one
    stream.leading = leading;
    stream.trailing = trailing;
    stream.first_is_raw = false;
    meaningful = raw ? 32u : (silent ? 0u : meaningful);
    reader.consume(header_bits);
    reader.refill(ring, lane);
    const uint32_t payload = (uint32_t)((reader.buffer >> 1) >> (63u - meaningful)); // 0 bits: 0
    reader.consume(meaningful);
    const uint32_t bits = raw ? payload : (stream.last ^ (payload << (trailing & 31u)));
    stream.last = bits;
    return bits;
}

// Values of the two streams of segment i: the model's (MacaqueV segments only) and the residual tail's.
__device__ __forceinline__ void mv_stream_lengths(const DevSegments &s, uint64_t i, const uint32_t *known_totals,
                                                  uint32_t *n_model_values, uint32_t *n_residuals, uint32_t *n_model_points,
                                                  uint32_t *error) {
    const SegInfo info = analyse_segment(s, i, known_totals, nullptr, false);
    *error = info.error;
    const uint32_t n_res = info.desc.n_total - info.desc.n_model;
    *n_model_points = info.desc.n_model;
    *n_model_values = (info.desc.flags & FLAG_TYPE_MASK) == MDB_MACAQUE_V_ID ? info.desc.n_model : 0u;
    *n_residuals = n_res;
}

// ---- the same step for the kernels that decode one PIECE per lane, on 32-bit words -------------------------------
//
// ring_decode_value's step over a 64-bit buffer with a reader of its own per lane cost the wave 104 vector instructions
// per value (every shift, add and compare on 64 bits is two or three instructions, two refills per code each rotated
// four words through registers, the bit position was 64 bits wide). Here a lane keeps the three big-endian words its next code can reach into (a code is at most 45 bits:
// 13 of header, 32 of payload) and the bit offset into the first; header and payload come out of them with one funnel
// shift each, and the words behind them come from a ring of the lane's stream in LDS ([word][lane]: the lanes of a
// wave read different rows of their own column, two lanes per bank at worst), read at the top of the step and needed
// at its end. The ring is topped up for the whole wave from 16-byte chunks that were loaded one top-up earlier.
constexpr int PIECE_RING_WORDS = 16;
constexpr int PIECE_RING_ROWS = PIECE_RING_WORDS + 4; // (and four rows nobody reads: where a lane without room puts its chunk)
struct PieceReader {
    const uint4 *chunks; // 16-byte aligned; chunk k holds words [4 k, 4 k + 4) of the stream as this reader counts them
    uint32_t last_chunk; // the last one that holds payload (loads never go behind it)
    uint32_t loaded;     // words [.., loaded) have been put into the ring; a multiple of 4
    uint32_t word;       // index of w0
    uint32_t w0, w1, w2; // words word, word + 1, word + 2 (big endian: the stream's first bit on top)
    uint32_t shift;      // bits of w0 already consumed (0..31)
    uint4 ahead, further, beyond, last; // chunks loaded / 4 .. loaded / 4 + 3, on their way from memory

    __device__ __forceinline__ uint4 load(uint32_t index) const { return load_global(chunks + min(index, last_chunk)); }
    // nbytes > 0
    __device__ __forceinline__ void open(const uint8_t *bytes, uint64_t nbytes, uint64_t start_bit) {
        const uintptr_t address = reinterpret_cast<uintptr_t>(bytes);
        const uint32_t misalign = (uint32_t)(address & 15u);
        const uint64_t first_bit = 8ull * misalign + start_bit; // counted from the aligned base
        const uint64_t skipped = first_bit >> 7;                // whole chunks in front of it
        const uint64_t all_chunks = (nbytes + misalign + 15u) >> 4;
        chunks = reinterpret_cast<const uint4 *>(address - misalign) + skipped;
        last_chunk = (uint32_t)(all_chunks > skipped ? all_chunks - skipped - 1 : 0u);
        word = (uint32_t)((first_bit >> 5) & 3u);
        shift = (uint32_t)(first_bit & 31u);
    }
    // A lane without a piece runs through the same straight-line code as the others (nothing it makes is looked at):
    // its reader reads `anywhere`, 16 bytes that may be read.
    __device__ __forceinline__ void idle(const void *anywhere) {
        chunks = reinterpret_cast<const uint4 *>(reinterpret_cast<uintptr_t>(anywhere) & ~(uintptr_t)15u);
        last_chunk = 0;
        word = shift = 0;
    }
    __device__ __forceinline__ void begin() { // (every lane, after open() or idle())
        loaded = 0;
        w0 = w1 = w2 = 0;
        ahead = load(0);
        further = load(1);
        beyond = load(2);
        last = load(3);
    }
    // Can the next TWO values be decoded without another look? (a value moves up at most two words; the second one's
    // words behind w2 are rows word + 5 and word + 6 then)
    __device__ __forceinline__ bool hungry() const { return loaded < word + 7u; }
    // The whole wave, without a branch: every lane puts the chunk it has waited for into its column - behind what it
    // has there, or into rows nobody reads when there is no room for it (a lane far ahead of the hungry one) - and
    // asks for another one (the same one again when it could not place this one). Four chunks are under way: the one
    // placed now was asked for four top-ups - the time of a dozen values - ago.
    __device__ __forceinline__ void top_up(uint32_t (*ring)[MDB_WAVE], int lane) {
        const bool room = loaded <= word + ((uint32_t)PIECE_RING_WORDS - 4u);
        const uint32_t row = room ? loaded & (uint32_t)(PIECE_RING_WORDS - 1) : (uint32_t)PIECE_RING_WORDS;
        ring[row + 0][lane] = ahead.x;
        ring[row + 1][lane] = ahead.y;
        ring[row + 2][lane] = ahead.z;
        ring[row + 3][lane] = ahead.w;
        loaded += room ? 4u : 0u;
        auto move_up = [room](uint4 &to, const uint4 &from) {
            to.x = room ? from.x : to.x;
            to.y = room ? from.y : to.y;
            to.z = room ? from.z : to.z;
            to.w = room ? from.w : to.w;
        };
        move_up(ahead, further);
        move_up(further, beyond);
        move_up(beyond, last);
        last = load((loaded >> 2) + 3u);
    }
    // After the first top-ups: the three words the first code can reach into.
    __device__ __forceinline__ void start(const uint32_t (*ring)[MDB_WAVE], int lane) {
        w0 = __builtin_bswap32(ring[word][lane]);
        w1 = __builtin_bswap32(ring[word + 1u][lane]);
        w2 = __builtin_bswap32(ring[word + 2u][lane]);
    }
};

struct PieceState {
    uint32_t last;        // bits of the previous value
    uint32_t trailing;    // of the window the last `11` code opened
    uint32_t window_bits; // 32 - leading - trailing of that window (0: none yet - the index has seen every code: there is)
    bool raw;             // the next value is 32 raw bits (macaque_v.rs:289-293)
};

// The 32 bits that begin `shift` (0..31) bits into the 64 bits high:low.
__device__ __forceinline__ uint32_t bits_at(uint32_t high, uint32_t low, uint32_t shift) {
    return (uint32_t)(((((uint64_t)high) << 32) | low) << shift >> 32);
}

// One value (macaque_v.rs:297-322; the cursor index has seen every window of the stream: they are possible ones).
__device__ __forceinline__ uint32_t piece_decode_value(PieceReader &reader, PieceState &state, const uint32_t (*ring)[MDB_WAVE], int lane) {
    // (the two words that may move up, asked for now, needed last)
    const uint32_t behind0 = ring[(reader.word + 3u) & (uint32_t)(PIECE_RING_WORDS - 1)][lane];
    const uint32_t behind1 = ring[(reader.word + 4u) & (uint32_t)(PIECE_RING_WORDS - 1)][lane];
    const uint32_t head = bits_at(reader.w0, reader.w1, reader.shift); // the next 32 bits of the stream
    const uint32_t code = head >> 30;                                  // 0x: `0`, 2: `10`, 3: `11`
    const bool raw = state.raw;
    const bool opens = !raw && code == 3u, repeats = !raw && code == 2u;
    const uint32_t header_bits = raw ? 0u : ((0x0d020101u >> (code << 3)) & 15u);
    const uint32_t leading = (head >> 25) & 31u, length = (head >> 19) & 63u;
    state.trailing = opens ? (32u - length - leading) & 31u : state.trailing;
    state.window_bits = opens ? min(length, 32u) : state.window_bits;
    const uint32_t meaningful = raw ? 32u : (repeats ? 0u : state.window_bits);
    const uint32_t at = reader.shift + header_bits; // 0..44: where the payload begins, in bits from the top of w0
    const bool in_first = at < 32u;
    const uint32_t body = bits_at(in_first ? reader.w0 : reader.w1, in_first ? reader.w1 : reader.w2, at & 31u);
    const uint32_t payload = meaningful ? body >> ((32u - meaningful) & 31u) : 0u;
    const uint32_t bits = raw ? payload : (state.last ^ (payload << state.trailing));
    state.last = bits;
    state.raw = false;
    const uint32_t end = at + meaningful; // 0..76
    const uint32_t taken = end >> 5;      // whole words consumed: 0, 1 or 2
    reader.shift = end & 31u;
    reader.word += taken;
    const uint32_t up0 = __builtin_bswap32(behind0), up1 = __builtin_bswap32(behind1);
    const uint32_t n0 = taken == 0u ? reader.w0 : (taken == 1u ? reader.w1 : reader.w2);
    const uint32_t n1 = taken == 0u ? reader.w1 : (taken == 1u ? reader.w2 : up0);
    const uint32_t n2 = taken == 0u ? reader.w2 : (taken == 1u ? up0 : up1);
    reader.w0 = n0;
    reader.w1 = n1;
    reader.w2 = n2;
    return bits;
}

// The largest of the lanes' values, in every lane.
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
    for (int step = 1; step < MDB_WAVE; step <<= 1) x = max(x, (uint32_t)__shfl_xor((int)x, step, MDB_WAVE));
    return x;
}

// ---- what every piece kernel does before its first value -----------------------------------------------------------

struct PieceCursor { // an MvCursor (32 bytes) as the two uint4 it is loaded as
    uint4 c0, c1;
    __device__ __forceinline__ uint32_t bit_position() const { return c0.x; }
    __device__ __forceinline__ uint32_t xor_so_far() const { return c0.y; }
    __device__ __forceinline__ uint32_t segment() const { return c0.z; }
    __device__ __forceinline__ uint32_t point_index() const { return c0.w; }
    __device__ __forceinline__ uint32_t n_values() const { return c1.x; }
    __device__ __forceinline__ uint32_t chain_seed() const { return c1.z; }
    __device__ __forceinline__ uint32_t marks() const { return c1.w; } // (MvCursor::pad)
    __device__ __forceinline__ bool residual() const { return (c1.y & MV_WINDOW_RESIDUAL) != 0; }
};
__device__ __forceinline__ PieceCursor load_piece_cursor(const MvCursor *__restrict__ cursors, unsigned long long piece) {
    const uint4 *from = reinterpret_cast<const uint4 *>(cursors + piece);
    return PieceCursor{load_global(from), load_global(from + 1)};
}

// The reader on the piece's first code: in the values column of the cursor's segment or, for a tail, in its residuals
// column without the last byte. values_first / residuals_first: first_buffer() of the two, asked for at the top of the
// kernel (see view_data()).
__device__ __forceinline__ void piece_open(PieceReader &reader, const DevSegments &s, const PieceCursor &cursor,
                                           const uint8_t *values_first, const uint8_t *residuals_first) {
    const bool residual = cursor.residual();
    const uint32_t i = cursor.segment();
    const DevCol &column = residual ? s.residuals : s.values;
    const uint4 view = column.views[i];
    const uint64_t nbytes = residual ? (uint64_t)view.x - 1u : (uint64_t)view.x;
    reader.open(view_data(column, i, view, residual ? residuals_first : values_first), nbytes, cursor.bit_position());
}

// The state in front of that code: the value before it - `seed` is what the caller's operator starts the stream from
// (the comment at k_mv_index_walk, mdb_grid.hip) - and the window the walk found open there.
__device__ __forceinline__ PieceState piece_state(const PieceCursor &cursor, uint32_t seed) {
    // (no window yet - leading 255 - is a window of no bits: the stream's first code opens one)
    const uint32_t window = cursor.c1.y, leading = window & 255u, trailing = (window >> 8) & 255u;
    return PieceState{seed ^ cursor.xor_so_far(), trailing & 31u, leading + trailing <= 32u ? 32u - leading - trailing : 0u,
                      (window & MV_WINDOW_RAW) != 0};
}
// ... and of a lane without a piece (its reader: PieceReader::idle).
__device__ __forceinline__ PieceState piece_state_idle() { return PieceState{0u, 0u, 0u, false}; }

// Every lane, opened or idle: four chunks asked for, two of them put into the ring, the first code's words in hand.
__device__ __forceinline__ void piece_start(PieceReader &reader, uint32_t (*ring)[MDB_WAVE], int lane) {
    reader.begin();
    reader.top_up(ring, lane);
    reader.top_up(ring, lane);
    reader.start(ring, lane);
}

} // namespace mdb
