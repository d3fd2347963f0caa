// mdb_mask.hpp - row masks on the device: the bits of a mask (RowBits) and the points of one segment that a mask
// selects, aggregated without materialising them (segment_rows: segment_range of mdb_agg_dev.hpp with a predicate
// that sees the ROW of a point instead of its value). Shared by mdb_mask.hip and the masked aggregate of mdb_agg.hip.
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

// Aggregate the points of segment i whose timestamp lies in [t_lo, t_hi] and whose row is set in `bits`; the
// segment's first point inside the range is row `first_row`. The passes over the streams are segment_range's.
__device__ __forceinline__ void segment_rows(const DevSegments &s, uint64_t i, const SegInfo &info, int64_t t_lo,
                                             int64_t t_hi, uint64_t first_row, const RowBits &bits, RangeAcc &acc,
                                             uint32_t *error) {
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint32_t n_res = d.n_total - d.n_model;
    if (!(d.flags & FLAG_REGULAR)) {
        if (end < t_lo || d.start > t_hi) return;
        const uint4 vt = s.timestamps.views[i];
        const uint8_t *ts_bytes = view_data(s.timestamps, i, vt);
        if (type != MDB_MACAQUE_V_ID && n_res == 0) {
            uint64_t row = first_row;
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t, int64_t t) {
                if (t >= t_lo && t <= t_hi) {
                    if (bits.test(row)) acc.point(model_value_at(d, type, t));
                    row += 1;
                }
            });
            return;
        }
        // The index interval of the in-range timestamps first (they are sorted), then the values once.
        uint32_t k_lo = 0xffffffffu, k_hi = 0;
        decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t k, int64_t t) {
            if (t >= t_lo && t <= t_hi) {
                if (k < k_lo) k_lo = k;
                if (k > k_hi) k_hi = k;
            }
        });
        if (k_lo == 0xffffffffu) return;
        auto selected = [&](uint32_t k) { return k >= k_lo && k <= k_hi && bits.test(first_row + (k - k_lo)); };
        float seed = d.value;
        if (type == MDB_MACAQUE_V_ID) {
            const uint4 vv = s.values.views[i];
            uint32_t last_bits = 0;
            decode_macaque_v(view_data(s.values, i, vv), vv.x, d.n_model, false, 0, error, [&](uint32_t k, uint32_t v) {
                if (selected(k)) acc.point(__uint_as_float(v));
                last_bits = v;
            });
            seed = __uint_as_float(last_bits);
        } else {
            decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, d.n_model, error, [&](uint32_t k, int64_t t) {
                if (selected(k)) acc.point(model_value_at(d, type, t));
            });
        }
        if (n_res > 0) {
            const uint4 vr = s.residuals.views[i];
            decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, n_res, true, __float_as_uint(seed), error,
                             [&](uint32_t k, uint32_t v) {
                                 if (selected(d.n_model + k)) acc.point(__uint_as_float(v));
                             });
        }
        return;
    }

    // Regular timestamps start + k * delta: the in-range indices are an interval [k_lo, k_hi]; point k is row
    // first_row + (k - k_lo).
    uint32_t k_lo = 0, k_hi = 0;
    if (!regular_index_interval(d.start, d.delta, d.n_total, t_lo, t_hi, &k_lo, &k_hi)) return;
    auto selected = [&](uint32_t k) { return k >= k_lo && k <= k_hi && bits.test(first_row + (k - k_lo)); };
    if (type != MDB_MACAQUE_V_ID && k_lo < d.n_model) model_rows(d, type, k_lo, min(k_hi, d.n_model - 1), first_row, bits, acc);
    float seed = d.value;
    if (type == MDB_MACAQUE_V_ID) {
        const uint4 vv = s.values.views[i];
        uint32_t last_bits = 0;
        // Decode only as far as needed unless the residual seed (last value) is needed too.
        const bool residuals_in_range = n_res > 0 && k_hi >= d.n_model;
        const uint32_t upto = residuals_in_range ? d.n_model : min(d.n_model, k_hi + 1);
        if (k_lo < d.n_model || residuals_in_range) {
            decode_macaque_v(view_data(s.values, i, vv), vv.x, upto, false, 0, error, [&](uint32_t k, uint32_t v) {
                if (selected(k)) acc.point(__uint_as_float(v));
                last_bits = v;
            });
        }
        seed = __uint_as_float(last_bits);
    }
    if (n_res > 0 && k_hi >= d.n_model) {
        const uint4 vr = s.residuals.views[i];
        const uint32_t upto = k_hi - d.n_model + 1;
        decode_macaque_v(view_data(s.residuals, i, vr), vr.x - 1, upto, true, __float_as_uint(seed), error,
                         [&](uint32_t k, uint32_t v) {
                             if (selected(d.n_model + k)) acc.point(__uint_as_float(v));
                         });
    }
}

// mdb_agg.hip: the points of a batch in HBM that `words` selects (n_words words in HBM; first_row: n entries in HBM)
// folded into *inout with the rules of agg_filter_run (the lock held, the device set).
int agg_mask_run(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const unsigned long long *first_row,
                 const unsigned long long *words, uint64_t n_words, uint32_t which_mask, mdb_agg_state *inout);

} // namespace mdb
