// mdb_select.hpp - the selection step of the per-bucket quantiles (mdb_quantile_buckets*): an order statistic of 32-bit
// keys pinned digit by digit, 8 + 8 + 8 + 8 bits from the top. Plain arithmetic, written once for the device
// (k_quantile_select, mdb_hist_buckets.hip) and for host code: the check program tests/hist_buckets_host drives it under
// the CPU sanitizers with passes made from plain arrays.
//
// A pass counts, per (cell, rank), the points whose key carries the prefix that rank has pinned so far, by the next
// digit of the key. The step takes those counts and the rank that remains inside the prefix, and gives the digit that
// holds the rank and the rank that remains inside that digit. After SELECT_PASSES passes the prefix is the key.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MDB_SELECT_FN __host__ __device__ __forceinline__
#else
#define MDB_SELECT_FN inline
#endif

namespace mdb {

constexpr uint32_t SELECT_DIGIT_BITS = 8;
constexpr uint32_t SELECT_DIGITS = 1u << SELECT_DIGIT_BITS;
constexpr uint32_t SELECT_PASSES = 32 / SELECT_DIGIT_BITS;

// The totalOrder key (a signed integer) as an unsigned one with the same order, and back: digits are taken of this.
MDB_SELECT_FN uint32_t select_ukey(int32_t key) { return (uint32_t)key ^ 0x80000000u; }
MDB_SELECT_FN int32_t select_key_of_ukey(uint32_t ukey) { return (int32_t)(ukey ^ 0x80000000u); }

// The bits of the unsigned key that pass `pass` (0-based) counts by lie above this shift.
MDB_SELECT_FN uint32_t select_shift(uint32_t pass) { return 32u - SELECT_DIGIT_BITS * (pass + 1u); }

// p = q * (N - 1) in f64: the ranks floor(p) and ceil(p), 0-based and at most N - 1 (quantile_ranks of mdb_hist.hpp;
// q in [0, 1] and N >= 1 are the caller's).
MDB_SELECT_FN void select_ranks(double q, uint64_t n_points, uint64_t *rank_lo, uint64_t *rank_hi) {
    const double p = q * (double)(n_points - 1);
    const double below = ::floor(p), above = ::ceil(p);
    const uint64_t last = n_points - 1;
    const uint64_t lo = below >= 18446744073709551616.0 ? last : (uint64_t)below;
    const uint64_t hi = above >= 18446744073709551616.0 ? last : (uint64_t)above;
    *rank_lo = lo < last ? lo : last;
    *rank_hi = hi < last ? hi : last;
}

// The step: counts[d] points carry digit d, `rank` (0-based, below the sum of the counts) is looked for. Returns the
// first digit whose running count exceeds the rank; *remaining is the rank among the points of that digit. A rank at
// or beyond the sum (never the case after a correct pass) gives the last digit that holds a point.
MDB_SELECT_FN uint32_t select_digit(const uint64_t *counts, uint32_t n_digits, uint64_t rank, uint64_t *remaining) {
    uint64_t running = 0;
    uint32_t last = 0;
    uint64_t before_last = 0;
    for (uint32_t d = 0; d < n_digits; d++) {
        const uint64_t c = counts[d];
        if (c == 0) continue;
        if (rank - running < c) {
            *remaining = rank - running;
            return d;
        }
        last = d;
        before_last = running;
        running += c;
    }
    *remaining = running > before_last ? running - before_last - 1 : 0;
    return last;
}

} // namespace mdb
