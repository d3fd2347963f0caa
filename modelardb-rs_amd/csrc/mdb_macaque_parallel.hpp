// mdb_macaque_parallel.hpp - decoding ONE long MacaqueV value stream with many lanes.
//
// macaque_v::grid (crates/modelardb_compression/src/models/macaque_v.rs:272-323) is sequential by
// construction: value i's position in the bit stream depends on every earlier code, and its bits
// are XORed onto value i-1. One lane per stream (k_grid_serial) therefore runs at the latency of a
// single wave, and lossless data (BASELINE config 1: every chunk becomes one 65 536-value MacaqueV
// segment) leaves most of the GPU idle. This file cuts a stream into pieces of MV_PIECE_BITS bits and
// decodes the pieces in parallel, still bit for bit the same values.
//
// What a parse needs from the past is small. Codes are `10` (repeat), `0` + n bits (n = "meaningful
// bits" of the current window) and `11` + 5 bits leading zeros + 6 bits n + n bits (a new window).
// WHERE the codes are therefore depends on (bit position, n) only; the leading zeros of the window
// matter for the values (how far the n bits are shifted), not for the positions, and a `11` code
// sets both from the stream itself.
//
//  * k_mv_chains: the lanes of a piece look for places in it from which the stream parses cleanly to
//    the end of the piece: speculative "chains". Round 0 starts piece 0 at the real beginning. Then,
//    since real streams settle on one window and consist of `0` and `10` codes only from there on,
//    the candidates are the first 45 bits of the piece (the longest code) combined with a guess for
//    n: the n at the end of the nearest earlier piece that has chains (k_mv_guess). Pieces that are
//    still without a chain try the `11` patterns near their start (those need nothing from the
//    past), and further rounds of guesses carry the windows found so far past one more change of n
//    each, until no piece is without a chain. Wrong candidates die within a few codes, with one
//    exception: a parse that is a few bits late keeps reading the (almost always zero) top bits of
//    the window as control bits; such late copies are recognised by their distance to another
//    chain on the grid of code boundaries. Per chain a few boundaries are recorded where the real
//    parse may join it, and per such boundary what only the real parse can interpret (MvTrack).
//  * k_mv_links: every chain is parsed on from the end of its piece until it stands on a boundary
//    that a chain of a later piece recorded with the same n: from there on the two parses visit
//    the same positions. The link notes that target and both chains' accumulators at the boundary.
//  * k_mv_walk: one wave per stream follows the links from piece 0, whose chain starts at the real
//    beginning. Every chain it visits is thereby proven to be on the real parse from the linked
//    boundary on. Along the way it carries the real window (from the last real `11` code) and turns
//    the accumulators into the index and the predecessor value each confirmed chain starts with.
//    Chains it never visits are ignored. A broken link (no partner within MV_MAX_TAIL_BITS, a
//    malformed stream) hands the whole stream back to k_grid_serial.
//  * k_mv_decode: one lane per confirmed piece decodes its values from its confirmed start (position,
//    real window, index, predecessor value) straight to their final positions.
// Nothing is assumed about the data: a speculative chain is only ever used from a boundary the real
// parse has been shown to pass with the same n, and every other situation falls back to the
// sequential decoder. Here: what the kernels and their callers share; the kernels and mv_pipeline: mdb_mv_parallel.hip.
#pragma once

#include "mdb_segment_dev.hpp"

#include <functional>

namespace mdb {

constexpr int MV_CHAINS = 4; // speculative chains kept per piece
constexpr int MV_HEAD = 4;   // boundaries recorded per chain
constexpr uint32_t MV_SCAN_BITS = 256;    // `11` patterns are looked for this far into a piece
constexpr uint32_t MV_MAX_CODE_BITS = 45; // 2 + 5 + 6 + 32
constexpr int MV_ROUNDS = 12;             // k_mv_chains launches at most (a round without work costs ~nothing)
enum : int { MV_ROUND_START = 0, MV_ROUND_GUESS = 1, MV_ROUND_SCAN = 2 };
// Piece 0 from the real start; guessed windows for everyone; `11` patterns for pieces that still have
// no chain; then rounds of guesses, each of which carries the windows found so far past one more
// change of n, until no piece is without a chain.
__device__ __host__ inline int mv_round_kind(int round) {
    return round == 0 ? MV_ROUND_START : (round == 2 ? MV_ROUND_SCAN : MV_ROUND_GUESS);
}
constexpr uint32_t MV_SHIFT_BITS = 8;     // how late a parse can be and still live on zero top bits
constexpr uint32_t MV_SETTLE_CODES = 8;   // codes after which a guessed chain is recorded and compared
constexpr uint32_t MV_NO_WINDOW = 0xffffu;
constexpr uint32_t MV_NO_LENGTH = 0xffu;
#ifndef MDB_MV_MAX_TAIL_BITS
#define MDB_MV_MAX_TAIL_BITS (1u << 16)
#endif
constexpr uint32_t MV_MAX_TAIL_BITS = MDB_MV_MAX_TAIL_BITS;
constexpr uint32_t MV_NONE = 0xffffffffu; // link: no partner found
constexpr uint32_t MV_END = 0xfffffffeu;  // link: parsed to the end of the stream

// One stream that qualifies (indexed like serial_ids).
struct MvSeg {
    const uint32_t *words;         // aligned base of the payload
    unsigned long long out_offset; // of the segment's first visible point in out_val
    uint32_t bias_bits;            // slack bits in front of the payload in words[0]
    uint32_t total_bits;
    uint32_t n_words;
    uint32_t n_model;     // values in the stream
    uint32_t first;       // first wanted value index
    uint32_t visible_end; // one past the last wanted value index
    uint32_t n_pieces;    // 0: the stream does not qualify
    uint32_t done;        // set by k_mv_walk: k_mv_decode handles it, k_grid_serial skips it
};

// A recorded code boundary of a chain: a place where the real parse may join it.
struct MvRec {
    uint32_t pos;   // bit position of the next code
    uint32_t state; // window there: leading | meaningful << 8, or MV_NO_WINDOW
    uint32_t count; // values the chain has decoded before it
};

// A chain while it is being followed, and what it has accumulated. A chain cannot know from where on
// it coincides with the real parse, nor whether the leading zeros of its window are real before it
// has read a `11` code AFTER that point. So for each of its recorded boundaries h it keeps apart:
// raw[h], the XOR of the unshifted bits of the `0` codes between boundary h and the next `11` code
// (only the real parse knows how far those are shifted), and snap[h], the value of x at that `11`
// code; x is the XOR of everything the chain decoded, shifted with its own windows, which are real
// from that `11` code on if the real parse joined at boundary h.
struct MvTrack {
    uint32_t pos;
    uint32_t state;
    uint32_t count;
    uint32_t x;
    uint32_t seen; // bit h: a `11` code has been read since boundary h
    uint32_t raw[MV_HEAD];
    uint32_t snap[MV_HEAD];
};

struct MvChain { // chains[piece * MV_CHAINS + c]
    uint32_t n_head; // recorded boundaries, 0: unused
    MvTrack end;     // the chain at its first boundary at or beyond the end of its piece
};

struct MvLink { // links[piece * MV_CHAINS + c]
    uint32_t target;     // id (piece * MV_CHAINS + c) of the chain this parse joins, MV_END or MV_NONE
    uint32_t into_head;  // which recorded boundary of the target it joins at
    uint32_t into_count; // values the target had decoded there
    MvTrack from;        // this parse at the shared boundary
};

struct MvStart {
    uint32_t valid;
    uint32_t pos, state;  // real window
    uint32_t first_index; // index of the first value this piece decodes
    uint32_t value_bits;  // the value before it
    uint32_t n_values;
};

struct MvPieceCount {
    const MvSeg *segs;
    __device__ uint64_t operator()(uint64_t slot) const { return segs[slot].n_pieces; }
};

// Random-access reader: bits [pos, pos + count) of the stream, MSB first, zeros past the end.
// A lane's 64 neighbours read pieces that lie MV_PIECE_BITS apart, so a word load per code would
// touch 64 cache lines per instruction, over and over. Each lane therefore copies the words it is
// going to walk over into LDS once, 16 bytes at a time (`stage`), laid out [word][lane] so that a
// row is conflict free whatever word each lane is at; words outside that window (a parse that runs
// on for several pieces) still come from global memory.
// How much of a piece a lane copies: all of it when the batch is small (few waves, each as fast as it
// can be), half or a quarter when there are more waves than fit next to each other with 38 KB of LDS
// each (what does not get staged comes from global memory as before).
constexpr uint32_t MV_STAGE_WORDS = MV_PIECE_BITS / 32 + 20; // a piece, 8 bits before it, ~600 bits after it
constexpr uint32_t MV_STAGE_WORDS_HALF = MV_PIECE_BITS / 64 + 20;
constexpr uint32_t MV_STAGE_WORDS_QUARTER = MV_PIECE_BITS / 128 + 20;

struct MvReader {
    const uint32_t *words;
    uint32_t n_words;
    uint32_t bias_bits;
    uint32_t total_bits;
    uint32_t cached_word;
    uint64_t cache;
    const uint32_t *staged; // LDS, this lane's column, already byte swapped; nullptr: nothing staged
    uint32_t staged_first;  // first staged word
    uint32_t staged_words;  // how many
    __device__ __forceinline__ void open(const MvSeg &seg) {
        words = seg.words;
        n_words = seg.n_words;
        bias_bits = seg.bias_bits;
        total_bits = seg.total_bits;
        cached_word = 0xfffffffeu; // never index - 1 of a real word
        cache = 0;
        staged = nullptr;
        staged_first = 0;
        staged_words = 0;
    }
    // Copies words [first, first + WORDS) around bit position `from_pos` into `column` (this lane's
    // column of a [WORDS][MDB_WAVE] LDS array). Only this lane reads it back.
    template <uint32_t WORDS> __device__ __forceinline__ void stage(uint32_t *column, uint32_t from_pos) {
        // First staged word: at or before the word of from_pos, on a 16-byte boundary of the ADDRESS
        // (the payload itself is only byte aligned) so that the copy can use 16-byte loads.
        const uint32_t skew = (uint32_t)((reinterpret_cast<uintptr_t>(words) >> 2) & 3u);
        const uint32_t wanted = (bias_bits + from_pos) >> 5;
        const uint32_t rounded = (wanted + skew) & ~3u;
        const bool aligned = rounded >= skew;
        const uint32_t first = aligned ? rounded - skew : 0u;
#pragma unroll 4
        for (uint32_t k = 0; k < WORDS / 4; k++) {
            const uint32_t index = first + 4 * k;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (aligned && index + 3 < n_words) {
                v = *reinterpret_cast<const uint4 *>(words + index);
            } else {
                if (index < n_words) v.x = words[index];
                if (index + 1 < n_words) v.y = words[index + 1];
                if (index + 2 < n_words) v.z = words[index + 2];
                if (index + 3 < n_words) v.w = words[index + 3];
            }
            column[(4 * k + 0) * MDB_WAVE] = __builtin_bswap32(v.x);
            column[(4 * k + 1) * MDB_WAVE] = __builtin_bswap32(v.y);
            column[(4 * k + 2) * MDB_WAVE] = __builtin_bswap32(v.z);
            column[(4 * k + 3) * MDB_WAVE] = __builtin_bswap32(v.w);
        }
        staged = column;
        staged_first = first;
        staged_words = WORDS / 4 * 4;
    }
    __device__ __forceinline__ uint32_t word(uint32_t index) const {
        const uint32_t k = index - staged_first;
        if (k < staged_words) return staged[k * MDB_WAVE];
        return index < n_words ? __builtin_bswap32(words[index]) : 0u;
    }
    // count in [0, 32]
    __device__ __forceinline__ uint32_t peek(uint32_t pos, uint32_t count) {
        if (count == 0) return 0;
        const uint32_t at = bias_bits + pos;
        const uint32_t index = at >> 5;
        if (index != cached_word) {
            // Moving one word forward is the common case: reuse the low half.
            const uint32_t high = index == cached_word + 1 ? (uint32_t)cache : word(index);
            cache = ((uint64_t)high << 32) | word(index + 1);
            cached_word = index;
        }
        return (uint32_t)((cache << (at & 31u)) >> (64u - count));
    }
};

enum : int { MV_OK = 0, MV_MALFORMED = 1, MV_OVERRUN = 2 };
enum : uint32_t { MV_CODE_BITS = 0, MV_CODE_REPEAT = 1, MV_CODE_WINDOW = 2 };

__device__ __forceinline__ bool mv_valid_window(uint32_t leading, uint32_t meaningful) {
    // macaque_v.rs:305-313 as decode_macaque_v checks it: meaningful <= 32 and trailing <= 31.
    return meaningful <= 32u && leading + meaningful <= 32u && leading + meaningful >= 1u;
}

__device__ __forceinline__ uint32_t mv_length(uint32_t state) { return state >> 8; }

__device__ __forceinline__ uint32_t mv_shifted(uint32_t bits, uint32_t state) {
    const uint32_t trailing = 32u - (state >> 8) - (state & 0xffu);
    return bits << (trailing & 31u);
}

// Decodes the code at `pos` under window `state`; on MV_OK pos / state are advanced, `kind` says
// which code it was and `bits` holds its unshifted payload. Nothing is changed otherwise.
__device__ __forceinline__ int mv_step(MvReader &r, uint32_t &pos, uint32_t &state, uint32_t &kind,
                                       uint32_t &bits) {
    const uint32_t top = r.peek(pos, 13); // c0 c1 leading[5] meaningful[6]
    uint32_t header, meaningful, next_state = state;
    if ((top >> 12) == 0) { // `0`: the previous window again
        if (state == MV_NO_WINDOW) return MV_MALFORMED;
        header = 1;
        meaningful = state >> 8;
        kind = MV_CODE_BITS;
    } else if ((top >> 11) == 2) { // `10`: the value repeats
        if (pos + 2 > r.total_bits) return MV_OVERRUN;
        pos += 2;
        kind = MV_CODE_REPEAT;
        bits = 0;
        return MV_OK;
    } else { // `11` + window
        const uint32_t leading = (top >> 6) & 31u;
        meaningful = top & 63u;
        if (!mv_valid_window(leading, meaningful)) return MV_MALFORMED;
        header = 13;
        next_state = leading | (meaningful << 8);
        kind = MV_CODE_WINDOW;
    }
    if (pos + header + meaningful > r.total_bits) return MV_OVERRUN;
    bits = r.peek(pos + header, meaningful);
    pos += header + meaningful;
    state = next_state;
    return MV_OK;
}

// One code of a chain that has n_head recorded boundaries: like mv_step, plus the accumulators.
__device__ __forceinline__ int mv_track_step(MvReader &r, MvTrack &t, uint32_t n_head) {
    uint32_t kind = 0, bits = 0;
    const int rc = mv_step(r, t.pos, t.state, kind, bits);
    if (rc != MV_OK) return rc;
    t.count += 1;
    if (kind == MV_CODE_WINDOW) {
#pragma unroll
        for (uint32_t h = 0; h < MV_HEAD; h++)
            if (h < n_head && !((t.seen >> h) & 1u)) {
                t.snap[h] = t.x;
                t.seen |= 1u << h;
            }
    } else if (kind == MV_CODE_BITS) {
#pragma unroll
        for (uint32_t h = 0; h < MV_HEAD; h++)
            if (h < n_head && !((t.seen >> h) & 1u)) t.raw[h] ^= bits;
    }
    if (kind != MV_CODE_REPEAT) t.x ^= mv_shifted(bits, t.state);
    return MV_OK;
}

__device__ __forceinline__ MvTrack mv_track_at(uint32_t pos, uint32_t state) {
    MvTrack t;
    t.pos = pos;
    t.state = state;
    t.count = 0;
    t.x = 0;
    t.seen = 0;
#pragma unroll
    for (int h = 0; h < MV_HEAD; h++) t.raw[h] = t.snap[h] = 0;
    return t;
}

// Last slot whose first piece is <= piece (slots without pieces share the base of the next one).
__device__ __forceinline__ uint32_t mv_slot_of(const unsigned long long *piece_base, uint64_t n_slots,
                                               uint64_t piece) {
    uint64_t lo = 0, hi = n_slots;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (piece_base[mid] <= piece) lo = mid;
        else hi = mid;
    }
    return (uint32_t)lo;
}

// What the decoder needs to know about the stream of segment i: nothing (n_pieces 0) unless it
// qualifies. out_offset: where the value of its first visible point goes.
__device__ __forceinline__ MvSeg mv_describe(const DevSegments &s, uint64_t i, const SegInfo &info, uint32_t min_values,
                                             unsigned long long out_offset) {
    const uint4 view = s.values.views[i];
    MvSeg seg;
    seg.words = nullptr;
    seg.out_offset = 0;
    seg.bias_bits = seg.total_bits = seg.n_words = seg.n_model = seg.first = seg.visible_end = 0;
    seg.n_pieces = 0;
    seg.done = 0;
    if (mv_qualifies(info, view.x, min_values)) {
        const uint8_t *bytes = view_data(s.values, i, view);
        const uintptr_t address = reinterpret_cast<uintptr_t>(bytes);
        const uint32_t misalign = (uint32_t)(address & 3u);
        seg.words = reinterpret_cast<const uint32_t *>(address - misalign);
        seg.bias_bits = 8u * misalign;
        seg.total_bits = 8u * view.x;
        seg.n_words = (view.x + misalign + 3u) >> 2;
        seg.n_model = info.desc.n_model;
        seg.first = info.desc.first;
        seg.visible_end = info.desc.first + info.desc.n_visible;
        seg.out_offset = out_offset;
        seg.n_pieces = (seg.total_bits + MV_PIECE_BITS - 1) / MV_PIECE_BITS;
    }
    return seg;
}

// mdb_mv_parallel.hip: the decoder over n_serial candidate streams holding stream_bytes bytes between them (see there).
int mv_pipeline(mdb_ctx *ctx, uint64_t n_serial, uint64_t stream_bytes, bool forced, const std::function<void(MvSeg *)> &select,
                float *out_val, unsigned int *error, MvSeg **segs_out);

} // namespace mdb
