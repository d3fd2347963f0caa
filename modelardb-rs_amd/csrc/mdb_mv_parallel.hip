// mdb_mv_parallel.hip - the kernels of the speculative MacaqueV decoder (mdb_macaque_parallel.hpp says how it works)
// and mv_pipeline, the host driver that runs them for the grid (mdb_grid.hip) and for the aggregates (mdb_agg_mv.hip).
#include "mdb_macaque_parallel.hpp"
#include "mdb_scan.hpp"

namespace mdb {

#ifdef MDB_MV_DEBUG
__device__ unsigned long long mv_debug_counters[4]; // iterations, steps, max iterations of a lane, max ticks of a lane
#endif

// ---- k_mv_chains: MV_CHAINS lanes per piece -----------------------------------------------------------------
//
// guesses[piece]: up to two candidate n (one per byte, MV_NO_LENGTH = none); tried[piece]: the n this
// piece has already been searched with (one per byte, low three bytes) and, in the top byte, 0x01
// once a chain found with a guessed n is kept; pending[r]: pieces without any chain after round r.
//
// Several chains can survive a piece: in a stream of `0` codes of one length a parse that is a few
// bits late keeps reading the (almost always zero) top bits of the window as control bits and never
// notices, and parses that start early can hop onto such a late grid through a `10` code. They
// cannot be told apart for certain locally, so each of the MV_CHAINS lanes of a piece tries every
// MV_CHAINS-th entry point and keeps the first chain that survives; the real parse is usually among
// them, and k_mv_links / k_mv_walk find out which. A lane tries its candidates as ONE loop in which
// it either picks the next candidate or advances the current one by a code.

__device__ __forceinline__ bool mv_byte_listed(uint32_t list, uint32_t value) {
    for (int k = 0; k < 3; k++)
        if (((list >> (8 * k)) & 0xffu) == value) return true;
    return false;
}

template <uint32_t STAGE_WORDS>
__global__ __launch_bounds__(MDB_WAVE) void k_mv_chains(const MvSeg *__restrict__ segs,
                                                        const unsigned long long *__restrict__ piece_base,
                                                        uint64_t n_slots, int round,
                                                        const uint32_t *__restrict__ guesses,
                                                        uint32_t *__restrict__ tried, uint32_t *__restrict__ pending,
                                                        MvRec *__restrict__ heads, MvChain *__restrict__ chains) {
    __shared__ uint32_t stage_lds[STAGE_WORDS][MDB_WAVE];
    const uint64_t lane_id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t piece = lane_id / MV_CHAINS;
    const uint32_t sub = (uint32_t)(lane_id % MV_CHAINS);
    const int kind = mv_round_kind(round);
    // No lane leaves before the ballot at the end; `present` lanes have a piece.
    const bool present = piece < piece_base[n_slots] && !(round > 1 && pending[round - 1] == 0);
    MvChain *__restrict__ mine = chains + piece * MV_CHAINS; // the piece's chains; this lane owns [sub]
    MvRec *__restrict__ head = heads + (piece * MV_CHAINS + sub) * MV_HEAD;
    bool work = false, slot_used = false, piece_has_chain = false;
    uint32_t p = 0, piece_begin = 0, piece_end = 0;
    MvSeg seg;
    seg.total_bits = 0;
    MvReader reader;
    uint32_t tried_here = 0xffffffffu;
    if (present) {
        const uint32_t slot = mv_slot_of(piece_base, n_slots, piece);
        seg = segs[slot];
        p = (uint32_t)(piece - piece_base[slot]);
        reader.open(seg);
        piece_begin = p * MV_PIECE_BITS;
        piece_end = min(piece_begin + MV_PIECE_BITS, seg.total_bits);
        if (kind == MV_ROUND_START) {
            mine[sub].n_head = 0;
            if (sub == 0) tried[piece] = 0xffffffffu;
            work = p == 0 && sub == 0 && seg.total_bits >= 32;
        } else {
            for (uint32_t c = 0; c < MV_CHAINS; c++) piece_has_chain = piece_has_chain || mine[c].n_head > 0;
            slot_used = mine[sub].n_head > 0;
            tried_here = tried[piece];
            if (kind == MV_ROUND_SCAN) {
                work = p > 0 && !piece_has_chain;
            } else {
                // A guess this piece has not been searched with yet; once a chain found with a guessed
                // window is kept the piece stops searching.
                bool untried = false;
                for (int g = 0; g < 2; g++) {
                    const uint32_t candidate = (guesses[piece] >> (8 * g)) & 0xffu;
                    untried = untried || (candidate <= 32u && !mv_byte_listed(tried_here, candidate));
                }
                work = p > 0 && untried && (tried_here >> 24) != 0x01u;
            }
        }
    }
    // Every lane of a piece walks over the same bits: each keeps its own copy (a column of the array).
    if (work) reader.template stage<STAGE_WORDS>(&stage_lds[0][threadIdx.x], piece_begin);

    int guess_index = -1;           // which guess is being searched (guess rounds)
    uint32_t length = MV_NO_LENGTH; // its n, MV_NO_LENGTH: candidates are `11` patterns / the real start
    uint32_t o = 0, o_end = 0;      // next and last+1 entry point of this lane
    bool searching = work, running = false, found_with_guess = false;
    MvTrack at = mv_track_at(0u, 0u);
    uint32_t steps = 0, n_head = 0;
    if (work && kind == MV_ROUND_START) {
        // The real start: 32 raw bits of the first value, then codes, no window yet.
        at = mv_track_at(32u, MV_NO_WINDOW);
        head[0] = {32u, MV_NO_WINDOW, 0u};
        n_head = 1;
        running = true;
    } else if (work && kind == MV_ROUND_SCAN) {
        o = piece_begin + sub;
        o_end = min(piece_begin + MV_SCAN_BITS, piece_end);
    }
#ifdef MDB_MV_DEBUG
    unsigned long long debug_iterations = 0, debug_steps = 0;
    const unsigned long long debug_t0 = wall_clock64();
#endif
    while (searching) {
#ifdef MDB_MV_DEBUG
        debug_iterations += 1;
        debug_steps += running ? 1 : 0;
#endif
        if (!running) {
            if (slot_used) {
                searching = false; // this lane's slot is taken: one chain per lane
            } else if (o >= o_end) {
                // The next guess, if any.
                length = MV_NO_LENGTH;
                while (kind == MV_ROUND_GUESS && ++guess_index < 2) {
                    const uint32_t candidate = (guesses[piece] >> (8 * guess_index)) & 0xffu;
                    if (candidate > 32u || mv_byte_listed(tried_here, candidate)) continue;
                    length = candidate;
                    break;
                }
                if (length == MV_NO_LENGTH) {
                    searching = false;
                } else {
                    tried_here = (tried_here & 0xff000000u) | ((tried_here << 8) & 0x00ffff00u) | length;
                    // The real parse enters the piece within its first 45 bits. The leading zeros of
                    // the guessed window are unknown (and not needed: see MvTrack).
                    o = piece_begin + sub;
                    o_end = min(piece_begin + MV_MAX_CODE_BITS, piece_end);
                }
            } else if (length == MV_NO_LENGTH) { // a scan: is there a plausible `11` code at o?
                if (o + 13 <= seg.total_bits) {
                    const uint32_t top = reader.peek(o, 13);
                    if ((top >> 11) == 3u && mv_valid_window((top >> 6) & 31u, top & 63u)) {
                        at = mv_track_at(o, MV_NO_WINDOW);
                        steps = 0;
                        n_head = 0;
                        running = true;
                    }
                }
                o += MV_CHAINS;
            } else {
                at = mv_track_at(o, length << 8);
                steps = 0;
                n_head = 0;
                running = true;
                o += MV_CHAINS;
            }
        } else {
            // A candidate is followed to the first boundary at or beyond the end of the piece and kept
            // unless it is malformed. A guessed chain may only fall in step with the real parse after
            // a few codes, so its boundaries are recorded once it has settled.
            bool finished = at.pos >= piece_end;
            if (!finished) {
                const int rc = mv_track_step(reader, at, n_head);
                if (rc == MV_MALFORMED) {
                    running = false;
                } else if (rc == MV_OVERRUN) {
                    finished = true; // only padding is left: the chain reaches the end
                } else {
                    steps += 1;
                    const bool guessed = length != MV_NO_LENGTH;
                    if ((!guessed || steps >= MV_SETTLE_CODES) && n_head < MV_HEAD)
                        head[n_head++] = {at.pos, at.state, at.count};
                    finished = at.pos >= piece_end;
                }
            }
            if (finished) {
                if (n_head > 0) {
                    mine[sub].n_head = n_head;
                    mine[sub].end = at;
                    slot_used = true;
                    found_with_guess = length != MV_NO_LENGTH;
                }
                running = false;
            }
        }
    }
#ifdef MDB_MV_DEBUG
    atomicAdd(&mv_debug_counters[0], debug_iterations);
    atomicAdd(&mv_debug_counters[1], debug_steps);
    atomicMax(&mv_debug_counters[2], debug_iterations);
    atomicMax(&mv_debug_counters[3], wall_clock64() - debug_t0);
#endif
    // Bookkeeping per piece: its MV_CHAINS lanes sit next to each other in the wave.
    const uint64_t group = 0xfull << (4u * (threadIdx.x / MV_CHAINS));
    static_assert(MV_CHAINS == 4, "the group mask above assumes four lanes per piece");
    // A chain that ends 1..MV_SHIFT_BITS bits behind another chain of the piece on the same grid
    // (same n, a whole number of `0` codes apart) is a late copy of it: it lives on the zero top bits
    // of the window, never meets the real parse and would only cost k_mv_links a long walk.
    {
        const bool kept_now = present && work && slot_used && n_head > 0 && found_with_guess;
        const uint32_t my_pos = at.pos, my_state = at.state;
        bool late_copy = false;
        for (int other = 0; other < MV_CHAINS; other++) {
            const int source = (int)(threadIdx.x / MV_CHAINS) * MV_CHAINS + other;
            const uint32_t their_pos = __shfl(my_pos, source, MDB_WAVE);
            const uint32_t their_state = __shfl(my_state, source, MDB_WAVE);
            const bool their_kept = __shfl((int)kept_now, source, MDB_WAVE) != 0;
            if (!kept_now || !their_kept || other == (int)sub) continue;
            if (mv_length(their_state) != mv_length(my_state) || mv_length(my_state) > 32u) continue;
            const uint32_t code_bits = 1u + mv_length(my_state);
            const uint32_t lag = (my_pos + code_bits * 256u - their_pos) % code_bits;
            late_copy = late_copy || (lag >= 1 && lag <= MV_SHIFT_BITS);
        }
        if (late_copy) {
            mine[sub].n_head = 0;
            slot_used = false;
            found_with_guess = false;
        }
    }
    const bool any_chain = (__ballot(present && slot_used) & group) != 0;
    const bool any_guessed = (__ballot(found_with_guess) & group) != 0;
    if (present && sub == 0) {
        if (work && kind == MV_ROUND_GUESS)
            tried[piece] = (tried_here & 0x00ffffffu) | (any_guessed || (tried_here >> 24) == 0x01u ? 0x01000000u : 0xff000000u);
        if (!any_chain) atomicAdd(&pending[round], 1u);
    }
}

// ---- k_mv_guess: one wave per entry of the serial list ----------------------------------------------------
//
// guesses[piece] = the n at the end of the chains of the nearest earlier piece of the stream that
// has chains (two of them, if its chains disagree).
__global__ __launch_bounds__(MDB_WAVE) void k_mv_guess(const MvSeg *__restrict__ segs,
                                                       const unsigned long long *__restrict__ piece_base,
                                                       const MvChain *__restrict__ chains,
                                                       uint32_t *__restrict__ guesses) {
    const uint64_t slot = blockIdx.x;
    const uint32_t n_pieces = segs[slot].n_pieces;
    if (n_pieces == 0) return;
    const int lane = threadIdx.x;
    const uint64_t first_piece = piece_base[slot];
    uint32_t carry = MV_NONE; // uniform: the answer of the last piece with chains in earlier groups of 64
    for (uint32_t base = 0; base < n_pieces; base += MDB_WAVE) {
        const uint32_t q = base + lane;
        uint32_t seen = MV_NONE;
        if (q < n_pieces) {
            const MvChain *__restrict__ theirs = chains + (first_piece + q) * MV_CHAINS;
            bool has_chain = false;
            for (int c = 0; c < MV_CHAINS; c++) has_chain = has_chain || theirs[c].n_head > 0;
            if (has_chain) {
                // The chains found last first: those come from guessed windows, which are right more
                // often than the survivors of a scan for `11` patterns.
                uint32_t a = MV_NO_LENGTH, b = MV_NO_LENGTH;
                for (int c = MV_CHAINS - 1; c >= 0; c--) {
                    if (theirs[c].n_head == 0) continue;
                    const uint32_t length = mv_length(theirs[c].end.state) & 0xffu;
                    if (a == MV_NO_LENGTH) a = length;
                    else if (b == MV_NO_LENGTH && length != a) b = length;
                }
                seen = 0xffff0000u | (b << 8) | a;
            }
        }
        // Inclusive "last one seen at or before this lane".
        uint32_t inclusive = seen;
#pragma unroll
        for (int delta = 1; delta < MDB_WAVE; delta <<= 1) {
            const uint32_t up = __shfl_up(inclusive, delta, MDB_WAVE);
            if (lane >= delta && inclusive == MV_NONE) inclusive = up;
        }
        uint32_t before = __shfl_up(inclusive, 1, MDB_WAVE);
        if (lane == 0 || before == MV_NONE) before = carry; // nothing earlier in this group of pieces
        if (q < n_pieces) guesses[first_piece + q] = before;
        const uint32_t last = __shfl(inclusive, MDB_WAVE - 1, MDB_WAVE);
        if (last != MV_NONE) carry = last;
    }
}

// ---- k_mv_links: one lane per chain ---------------------------------------------------------------------

__global__ __launch_bounds__(MDB_WAVE) void k_mv_links(const MvSeg *__restrict__ segs,
                                                       const unsigned long long *__restrict__ piece_base,
                                                       uint64_t n_slots, const MvRec *__restrict__ heads,
                                                       const MvChain *__restrict__ chains,
                                                       MvLink *__restrict__ links) {
    const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t piece = id / MV_CHAINS;
    if (piece >= piece_base[n_slots]) return;
    MvLink link;
    link.target = MV_NONE;
    link.into_head = 0;
    link.into_count = 0;
    link.from = mv_track_at(0u, 0u);
    const uint32_t n_head = chains[id].n_head;
    if (n_head > 0) {
        const uint32_t slot = mv_slot_of(piece_base, n_slots, piece);
        const MvSeg seg = segs[slot];
        const uint64_t first_piece = piece_base[slot];
        const uint32_t p = (uint32_t)(piece - first_piece);
        MvReader reader;
        reader.open(seg);
        MvTrack at = chains[id].end;
        const uint32_t tail_begin = at.pos;
        uint32_t partner = 0xffffffffu, partner_last_pos = 0;
        while (true) {
            const uint32_t r = at.pos / MV_PIECE_BITS;
            if (at.pos >= seg.total_bits || r >= seg.n_pieces) {
                link.target = MV_END;
                break;
            }
            if (r != partner) {
                // Only later pieces can be joined (a chain that ends in the padding of the last piece
                // still stands inside its own piece). Their recorded boundaries all lie near the start
                // of the piece: note where they end to stop looking early.
                partner = r;
                partner_last_pos = 0;
                if (r > p) {
                    for (uint32_t k = 0; k < MV_CHAINS; k++) {
                        const uint32_t n = chains[(first_piece + r) * MV_CHAINS + k].n_head;
                        if (n == 0) continue;
                        const uint32_t last = heads[((first_piece + r) * MV_CHAINS + k) * MV_HEAD + n - 1].pos;
                        partner_last_pos = max(partner_last_pos, last + 1);
                    }
                }
            }
            if (at.pos < partner_last_pos) {
                bool joined = false;
                for (uint32_t k = 0; k < MV_CHAINS && !joined; k++) {
                    const uint64_t other = (first_piece + r) * MV_CHAINS + k;
                    const uint32_t n = chains[other].n_head;
                    if (n == 0) continue;
                    for (uint32_t h = 0; h < n; h++) {
                        const MvRec rec = heads[other * MV_HEAD + h];
                        if (rec.pos != at.pos || mv_length(rec.state) != mv_length(at.state)) continue;
                        link.target = (uint32_t)other;
                        link.into_head = h;
                        link.into_count = rec.count;
                        joined = true;
                        break;
                    }
                }
                if (joined) break;
            }
            if (at.pos - tail_begin > MV_MAX_TAIL_BITS) break; // MV_NONE: the sequential decoder takes over
            const int rc = mv_track_step(reader, at, n_head);
            if (rc == MV_MALFORMED) break;
            if (rc == MV_OVERRUN) {
                link.target = MV_END;
                break;
            }
        }
        link.from = at;
    }
    links[id] = link;
}

// ---- k_mv_walk: one wave per entry of the serial list -------------------------------------------------------

__global__ __launch_bounds__(MDB_WAVE) void k_mv_walk(MvSeg *__restrict__ segs,
                                                      const unsigned long long *__restrict__ piece_base,
                                                      const MvChain *__restrict__ chains,
                                                      const MvLink *__restrict__ links,
                                                      MvStart *__restrict__ starts) {
    const uint64_t slot = blockIdx.x;
    const MvSeg seg = segs[slot];
    if (seg.n_pieces == 0) return;
    const int lane = threadIdx.x;
    const uint64_t first_piece = piece_base[slot];
    const uint64_t first_chain = first_piece * MV_CHAINS;
    const uint32_t n_ids = seg.n_pieces * MV_CHAINS;
    MvReader reader;
    reader.open(seg);
    bool ok = seg.total_bits >= 32 && seg.n_model >= 1 && chains[first_chain].n_head > 0;
    uint32_t q = 0;           // chain on the real parse, relative to first_chain (uniform)
    uint32_t first_index = 1; // value 0 is the raw first value
    uint32_t value_bits = reader.peek(0, 32);
    // Where the real parse entered chain q (position, real window, which recorded boundary of the
    // chain that is, how many values the chain had decoded there).
    uint32_t pos = 32, state = MV_NO_WINDOW, entered_head = 0, entered_count = 0;
    uint32_t window_first = 0;
    bool window_valid = false;
    MvLink window;
    window.target = MV_NONE;
    window.into_head = window.into_count = 0;
    window.from = mv_track_at(0u, 0u);
    while (ok) {
        if (!window_valid || q - window_first >= MDB_WAVE) {
            window_first = q;
            if (q + lane < n_ids) window = links[first_chain + q + lane];
            window_valid = true;
        }
        const int source = (int)(q - window_first);
        const uint32_t target = __shfl(window.target, source, MDB_WAVE);
        const uint32_t into_head = __shfl(window.into_head, source, MDB_WAVE);
        const uint32_t into_count = __shfl(window.into_count, source, MDB_WAVE);
        const uint32_t from_pos = __shfl(window.from.pos, source, MDB_WAVE);
        const uint32_t from_state = __shfl(window.from.state, source, MDB_WAVE);
        const uint32_t from_count = __shfl(window.from.count, source, MDB_WAVE);
        const uint32_t from_x = __shfl(window.from.x, source, MDB_WAVE);
        const uint32_t from_seen = __shfl(window.from.seen, source, MDB_WAVE);
        uint32_t from_raw = 0, from_snap = 0;
#pragma unroll
        for (uint32_t h = 0; h < MV_HEAD; h++) {
            const uint32_t raw_h = __shfl(window.from.raw[h], source, MDB_WAVE);
            const uint32_t snap_h = __shfl(window.from.snap[h], source, MDB_WAVE);
            if (h == entered_head) {
                from_raw = raw_h;
                from_snap = snap_h;
            }
        }
        if (target == MV_NONE) {
            ok = false;
            break;
        }
        const uint32_t left = seg.n_model - first_index;
        uint32_t n_values = target == MV_END ? left : from_count - entered_count;
        const bool last = target == MV_END || n_values >= left;
        if (n_values > left) n_values = left;
        if (lane == 0) starts[first_piece + q / MV_CHAINS] = {1u, pos, state, first_index, value_bits, n_values};
        if (last) break;
        const uint32_t next = target - (uint32_t)first_chain;
        if (next / MV_CHAINS <= q / MV_CHAINS || next >= n_ids) { // links only ever point to later pieces
            ok = false;
            break;
        }
        // The XOR of the values decoded between the two boundaries (see MvTrack): the `0` codes up
        // to the first `11` code carry bits that the REAL window at the entry shifts; from that `11`
        // on the chain's own shifts were real.
        const bool seen = (from_seen >> entered_head) & 1u;
        uint32_t delta = 0;
        if (from_raw != 0) {
            if (state == MV_NO_WINDOW) { // cannot happen: `0` codes need a window
                ok = false;
                break;
            }
            delta = mv_shifted(from_raw, state);
        }
        if (seen) {
            delta ^= from_x ^ from_snap;
            state = from_state; // set by a `11` code the real parse has read too
        }
        if (mv_length(state) != mv_length(from_state)) { // cannot happen: same positions, same n
            ok = false;
            break;
        }
        value_bits ^= delta;
        first_index += n_values;
        pos = from_pos;
        entered_head = into_head;
        entered_count = into_count;
        q = next;
    }
    if (lane == 0) segs[slot].done = ok ? 1u : 0u;
}

// ---- k_mv_decode: one lane per piece -----------------------------------------------------------------------

template <uint32_t STAGE_WORDS>
__global__ __launch_bounds__(MDB_WAVE) void k_mv_decode(const MvSeg *__restrict__ segs,
                                                        const unsigned long long *__restrict__ piece_base,
                                                        uint64_t n_slots, const MvStart *__restrict__ starts,
                                                        float *__restrict__ out_val,
                                                        unsigned int *__restrict__ error) {
    __shared__ uint32_t stage_lds[STAGE_WORDS][MDB_WAVE];
    const uint64_t piece = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (piece >= piece_base[n_slots]) return;
    const MvStart start = starts[piece];
    if (!start.valid) return;
    const uint32_t slot = mv_slot_of(piece_base, n_slots, piece);
    const MvSeg seg = segs[slot];
    if (!seg.done) return; // the sequential decoder handles this stream
    MvReader reader;
    reader.open(seg);
    reader.template stage<STAGE_WORDS>(&stage_lds[0][threadIdx.x], start.pos);
    float *__restrict__ out = out_val + seg.out_offset;
    uint32_t value = start.value_bits;
    if (piece == piece_base[slot] && seg.first == 0) out[0] = __uint_as_float(value); // the raw first value
    uint32_t pos = start.pos, state = start.state, index = start.first_index;
    for (uint32_t k = 0; k < start.n_values; k++, index++) {
        uint32_t kind = 0, bits = 0;
        if (mv_step(reader, pos, state, kind, bits) != MV_OK) {
            atomicOr(error, ERR_BITSTREAM);
            return;
        }
        if (kind != MV_CODE_REPEAT) value ^= mv_shifted(bits, state);
        if (index >= seg.first && index < seg.visible_end) out[index - seg.first] = __uint_as_float(value);
    }
}

// The parallel decoder over n_serial candidate streams holding stream_bytes
// bytes between them: `select` launches the kernel that fills segs[0..n_serial), the decoded values go
// to out_val + MvSeg::out_offset and MvSeg::done says which streams were decoded. *segs_out stays
// nullptr when the batch has so many streams that one lane per stream is the better plan.
int mv_pipeline(mdb_ctx *ctx, uint64_t n_serial, uint64_t stream_bytes, bool forced, const std::function<void(MvSeg *)> &select,
                float *out_val, unsigned int *error, MvSeg **segs_out) {
    // Every qualifying stream has ceil(bits / MV_PIECE_BITS) pieces.
    const uint64_t max_pieces = stream_bytes * 8 / MV_PIECE_BITS + n_serial + 1;
    if (max_pieces > MV_MAX_PIECES && !forced) return 0; // enough streams for one lane per stream
    if (max_pieces * MV_CHAINS > 0x7fffff00ull) return 0;
    const uint64_t sums_bytes = scan_block_sums_bytes(n_serial);
    const uint64_t segs_bytes = align_up(n_serial * sizeof(MvSeg), 256);
    const uint64_t base_bytes = align_up((n_serial + 1) * 8, 256) + align_up(sums_bytes, 256);
    const uint64_t heads_bytes = align_up(max_pieces * MV_CHAINS * MV_HEAD * sizeof(MvRec), 256);
    const uint64_t chains_bytes = align_up(max_pieces * MV_CHAINS * sizeof(MvChain), 256);
    const uint64_t links_bytes = align_up(max_pieces * MV_CHAINS * sizeof(MvLink), 256);
    const uint64_t starts_bytes = align_up(max_pieces * sizeof(MvStart), 256);
    const uint64_t guesses_bytes = 2 * align_up(max_pieces * 4, 256) + 256; // guesses + tried + pending
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_MV, segs_bytes + base_bytes + heads_bytes + chains_bytes + links_bytes +
                                            starts_bytes + guesses_bytes, &p))
        return 1;
    uint8_t *at = static_cast<uint8_t *>(p);
    MvSeg *segs = reinterpret_cast<MvSeg *>(at);
    at += segs_bytes;
    unsigned long long *piece_base = reinterpret_cast<unsigned long long *>(at);
    unsigned long long *block_sums = reinterpret_cast<unsigned long long *>(at + align_up((n_serial + 1) * 8, 256));
    at += base_bytes;
    MvRec *heads = reinterpret_cast<MvRec *>(at);
    at += heads_bytes;
    MvChain *chains = reinterpret_cast<MvChain *>(at);
    at += chains_bytes;
    MvLink *links = reinterpret_cast<MvLink *>(at);
    at += links_bytes;
    MvStart *starts = reinterpret_cast<MvStart *>(at);
    at += starts_bytes;
    uint32_t *guesses = reinterpret_cast<uint32_t *>(at);
    uint32_t *tried = reinterpret_cast<uint32_t *>(at + align_up(max_pieces * 4, 256));
    uint32_t *pending = reinterpret_cast<uint32_t *>(at + 2 * align_up(max_pieces * 4, 256));
    MDB_HIP_CHECK(hipMemsetAsync(pending, 0, 256, ctx->stream));
    MDB_HIP_CHECK(hipMemsetAsync(starts, 0, starts_bytes, ctx->stream));
    select(segs);
    if (device_exclusive_scan(ctx, MvPieceCount{segs}, n_serial, piece_base, block_sums, "k_mv_scan")) return 1;
    const uint32_t piece_blocks = (uint32_t)((max_pieces + MDB_WAVE - 1) / MDB_WAVE);
    // A wave that stages whole pieces takes 38 KB of LDS, so four of them fill a CU: beyond the
    // 1 024 waves that are resident at once, less staging and more waves is the better trade
    // (16 streams of 65 536 values: 5.8 / 5.95 / 6.0 ms with whole / half / quarter pieces staged;
    // 64 streams: 7.3 / 6.85 / 6.95 ms; 256 streams: 17.0 / 14.7 / 13.8 ms).
    const int staging = max_pieces <= 12288 ? 0 : (max_pieces <= 49152 ? 1 : 2);
    for (int round = 0; round < MV_ROUNDS; round++) {
        if (mv_round_kind(round) == MV_ROUND_GUESS) {
            LaunchTimer timer(ctx, "k_mv_guess");
            hipLaunchKernelGGL(k_mv_guess, dim3((uint32_t)n_serial), dim3(MDB_WAVE), 0, ctx->stream, segs,
                               piece_base, chains, guesses);
        }
        LaunchTimer timer(ctx, round == 0 ? "k_mv_chains_start" : (round == 1 ? "k_mv_chains_first" : "k_mv_chains_more"));
        const dim3 chain_grid((uint32_t)((max_pieces * MV_CHAINS + MDB_WAVE - 1) / MDB_WAVE));
        if (staging == 0)
            hipLaunchKernelGGL(k_mv_chains<MV_STAGE_WORDS>, chain_grid, dim3(MDB_WAVE), 0, ctx->stream, segs, piece_base,
                               n_serial, round, guesses, tried, pending, heads, chains);
        else if (staging == 1)
            hipLaunchKernelGGL(k_mv_chains<MV_STAGE_WORDS_HALF>, chain_grid, dim3(MDB_WAVE), 0, ctx->stream, segs,
                               piece_base, n_serial, round, guesses, tried, pending, heads, chains);
        else
            hipLaunchKernelGGL(k_mv_chains<MV_STAGE_WORDS_QUARTER>, chain_grid, dim3(MDB_WAVE), 0, ctx->stream, segs,
                               piece_base, n_serial, round, guesses, tried, pending, heads, chains);
    }
    {
        LaunchTimer timer(ctx, "k_mv_links");
        const uint32_t chain_blocks = (uint32_t)((max_pieces * MV_CHAINS + MDB_WAVE - 1) / MDB_WAVE);
        hipLaunchKernelGGL(k_mv_links, dim3(chain_blocks), dim3(MDB_WAVE), 0, ctx->stream, segs, piece_base,
                           n_serial, heads, chains, links);
    }
    {
        LaunchTimer timer(ctx, "k_mv_walk");
        hipLaunchKernelGGL(k_mv_walk, dim3((uint32_t)n_serial), dim3(MDB_WAVE), 0, ctx->stream, segs, piece_base,
                           chains, links, starts);
    }
    {
        LaunchTimer timer(ctx, "k_mv_decode");
        if (staging == 0)
            hipLaunchKernelGGL(k_mv_decode<MV_STAGE_WORDS>, dim3(piece_blocks), dim3(MDB_WAVE), 0, ctx->stream, segs,
                               piece_base, n_serial, starts, out_val, error);
        else if (staging == 1)
            hipLaunchKernelGGL(k_mv_decode<MV_STAGE_WORDS_HALF>, dim3(piece_blocks), dim3(MDB_WAVE), 0, ctx->stream, segs,
                               piece_base, n_serial, starts, out_val, error);
        else
            hipLaunchKernelGGL(k_mv_decode<MV_STAGE_WORDS_QUARTER>, dim3(piece_blocks), dim3(MDB_WAVE), 0, ctx->stream,
                               segs, piece_base, n_serial, starts, out_val, error);
    }
    *segs_out = segs;
    return 0;
}

} // namespace mdb
