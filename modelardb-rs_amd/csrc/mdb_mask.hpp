// mdb_mask.hpp - row masks on the device: the bits of a mask (RowBits), what a mask selects of a model's points
// (model_rows), and the two as a selector of segment_range (SegmentRows: mdb_agg_dev.hpp's walk with a test of the ROW
// of a point instead of its value). Shared by mdb_mask.hip and the masked aggregate of mdb_agg.hip.
//
// A mask over n_rows rows is ceil(n_rows / 64) 64-bit words; row r is bit r % 64 of word r / 64 (on a little-endian
// host an Arrow boolean bitmap byte for byte), bits at and beyond n_rows are zero. The rows are those of the range
// grid of a batch, in its order: segment i's rows are first_row[i] .. first_row[i] + rows[i] - 1.
#pragma once

#include "mdb_agg_dev.hpp"

namespace mdb {

struct RowBits {
    const unsigned long long *words;
    uint64_t n_words;
    // (r is below n_rows - the callers have checked that the batch has exactly n_rows rows; a row beyond the words: 0)
    __device__ __forceinline__ bool test(uint64_t r) const {
        return (r >> 6) < n_words && ((words[r >> 6] >> (r & 63)) & 1ull) != 0;
    }
    // The bits of rows r .. r + 63, row r in bit 0 (rows beyond the mask: 0).
    __device__ __forceinline__ unsigned long long window(uint64_t r) const {
        const uint64_t w = r >> 6;
        const uint32_t shift = (uint32_t)(r & 63);
        unsigned long long bits = w < n_words ? words[w] >> shift : 0ull;
        if (shift != 0 && w + 1 < n_words) bits |= words[w + 1] << (64 - shift);
        return bits;
    }
    // The set bits among rows r .. r + n - 1.
    __device__ __forceinline__ uint32_t count(uint64_t r, uint32_t n) const {
        uint32_t set = 0;
        for (uint32_t k = 0; k < n; k += 64) {
            unsigned long long bits = window(r + k);
            if (n - k < 64) bits &= (1ull << (n - k)) - 1ull;
            set += (uint32_t)__popcll(bits);
        }
        return set;
    }
};

// The selected ones of the model points [a, b] of a PMC-Mean or Swing segment with regular timestamps; point a is
// row `row_a`. The mask is walked 64 rows at a time: an all-zero window is skipped, a run of all-one windows goes
// through model_closed_form as one interval (a dense or an empty mask costs O(1) per 64 rows and one closed form per
// run), a mixed window is taken bit by bit (PMC-Mean needs only its popcount).
__device__ __forceinline__ void model_rows(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, uint64_t row_a,
                                           const RowBits &bits, RangeAcc &acc) {
    uint32_t run_a = 0, run_n = 0; // selected points not yet added: [run_a, run_a + run_n)
    uint32_t k = a;
    while (true) {
        const uint32_t n = min(64u, b - k + 1);
        const unsigned long long full = n == 64 ? ~0ull : (1ull << n) - 1ull;
        unsigned long long w = bits.window(row_a + (k - a)) & full;
        if (w == full) {
            if (run_n == 0) run_a = k;
            run_n += n;
        } else {
            if (run_n != 0) {
                model_closed_form(d, type, run_a, run_a + run_n - 1, acc);
                run_n = 0;
            }
            if (w != 0 && type == MDB_PMC_MEAN_ID) {
                const uint32_t set = (uint32_t)__popcll(w);
                acc.sum += (double)d.value * (double)set;
                acc.count += set;
                acc.min = min_num(acc.min, d.value);
                acc.max = max_num(acc.max, d.value);
            } else {
                while (w != 0) {
                    const uint32_t j = (uint32_t)__builtin_ctzll(w);
                    w &= w - 1;
                    acc.point(model_value_at(d, type, d.start + (int64_t)((uint64_t)(k + j) * (uint64_t)d.delta)));
                }
            }
        }
        if (b - k < 64) break;
        k += 64;
    }
    if (run_n != 0) model_closed_form(d, type, run_a, run_a + run_n - 1, acc);
}

// The selector of segment_range (mdb_agg_dev.hpp) for a mask: the segment's first point inside the range is row
// `first_row` of `bits`, a point counts when its row is set.
struct SegmentRows {
    static constexpr bool by_row = true;
    RowBits bits;
    uint64_t first_row;
    __device__ __forceinline__ bool counts(float, uint64_t row) const { return bits.test(first_row + row); }
    __device__ __forceinline__ void model(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, uint64_t row_a,
                                          RangeAcc &acc) const {
        model_rows(d, type, a, b, first_row + row_a, bits, acc);
    }
};

// mdb_agg.hip: the points of a batch in HBM that `words` selects (n_words words in HBM; first_row: n entries in HBM)
// folded into *inout with the rules of agg_filter_run (the lock held, the device set).
int agg_mask_run(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const unsigned long long *first_row,
                 const unsigned long long *words, uint64_t n_words, uint32_t which_mask, mdb_agg_state *inout);

} // namespace mdb
