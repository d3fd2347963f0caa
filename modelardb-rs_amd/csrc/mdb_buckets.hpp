// mdb_buckets.hpp - what the two operators over (segment, bucket) pairs share beyond mdb_agg_dev.hpp's bucket
// arithmetic: mdb_buckets.hip (COUNT / MIN / MAX / SUM per bucket) and mdb_m4.hip (first / last / min / max points per
// bucket). The sizes of the pair machinery, the visible values of a piece of an indexed MacaqueV stream, and the host
// steps that do not depend on what a partial holds (the span and its scan, the entry counts of the pieces, the sort of
// the keys, the check of a slice): defined in mdb_buckets.hip. What does depend on the partial - the reduction tree and
// the fold - is one template over it: mdb_bucket_fold.hpp.
#pragma once

#include "mdb_agg_dev.hpp"
#include "mdb_mv_pieces.hpp"

namespace mdb {

constexpr int BUCKET_THREADS = 256;
constexpr uint32_t BUCKET_TILE = 64;                    // entries per lane and level of the reduction tree
constexpr int BUCKET_MAX_LEVELS = 12;                   // 64^11 > 2^64
constexpr uint64_t BUCKET_SLICE_DEFAULT = 1ull << 24;   // pairs per slice: 512 MB of partials and keys
constexpr uint64_t BUCKET_SLICE_MAX = 1ull << 31;       // (pair numbers of the sort path are 32-bit)
constexpr uint32_t ERR_BUCKET_GROUP = 1u << 31;         // k_agg_bucket_span: a group id >= n_groups

// The visible values [from, upto) of the piece (segment-level indices) and the buckets [b_first, b_last] they reach;
// false: the piece is not taken or holds no visible value.
__device__ __forceinline__ bool bucket_piece_span(const DevSegments &s, const BucketRequest &r, const unsigned long long *piece_base,
                                                  const PieceCursor &cursor, SegInfo *info_out, uint32_t *from,
                                                  uint32_t *upto, uint64_t *b_first, uint64_t *b_last) {
    const uint32_t i = cursor.segment(), point_index = cursor.point_index(), n_values = cursor.n_values();
    const uint4 ts_view = s.timestamps.views[i];
    if ((int32_t)ts_view.x > 0 && (view_inline_byte(ts_view, 0) & 0x80u) != 0) return false; // (irregular: not taken)
    uint64_t unused = 0;
    if (bucket_span(s.start_time[i], s.end_time[i], r, &unused) == 0) return false;
    const SegInfo info = analyse_segment(s, i);
    if (!(cursor.residual() ? bucket_tail_by_pieces(s, i, info, piece_base) : bucket_values_by_pieces(s, i, info, piece_base)))
        return false;
    const int64_t lo = r.t_lo > r.origin ? r.t_lo : r.origin;
    const int64_t last = buckets_last_time(r);
    const int64_t hi = r.t_hi < last ? r.t_hi : last;
    uint32_t k_lo = 0, k_hi = 0;
    if (lo > hi || !regular_index_interval(info.desc.start, info.desc.delta, info.desc.n_total, lo, hi, &k_lo, &k_hi))
        return false;
    *from = max(k_lo, point_index);
    *upto = min(k_hi + 1, point_index + n_values);
    if (*from >= *upto) return false;
    const SegDesc &d = info.desc;
    const uint64_t width = (uint64_t)r.width;
    *b_first = ((uint64_t)(d.start + (int64_t)((uint64_t)*from * (uint64_t)d.delta)) - (uint64_t)r.origin) / width;
    *b_last = ((uint64_t)(d.start + (int64_t)((uint64_t)(*upto - 1) * (uint64_t)d.delta)) - (uint64_t)r.origin) / width;
    *info_out = info;
    return true;
}

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + BUCKET_THREADS - 1) / BUCKET_THREADS); }

// MDB_AGG_BUCKET_SLICE_PAIRS, or the default: the pairs (and piece entries) of one slice.
uint64_t slice_pairs_setting();

// An operator's own span kernel in place of k_agg_bucket_span (mdb_integral.hip: a segment's extent reaches over the
// link to its right neighbour): launch() enqueues it on the context's stream; it writes counts[i], the pairs of
// segment i, and ORs ERR_BUCKET_GROUP into *error for a group id that is not below n_groups, as k_agg_bucket_span does.
struct BucketSpanKernel {
    const char *name; // (of the launch, for mdb_profile_*)
    void (*launch)(mdb_ctx *ctx, const DevSegments &s, const uint32_t *groups, const BucketRequest &r,
                   unsigned long long *counts, unsigned int *error, const void *arg);
    const void *arg;
};

// k_agg_bucket_span (span nullptr; or the operator's own) and its scan over the device batch `in` (s = to_dev(in)):
// *offsets (n + 1, in scratch) are the pair offsets per segment, *words two zeroed read-back words (an error word, an
// "unsorted" flag) next to them, *total the number of pairs. Fails on a group id that is not below n_groups - on any
// row.
int bucket_span_pairs(mdb_ctx *ctx, const mdb_segments *in, const DevSegments &s, const uint32_t *groups,
                      const BucketRequest &r, const unsigned long long **offsets, unsigned int **words,
                      unsigned long long *total, const BucketSpanKernel *span = nullptr);

// The entries the pieces of the batch's cursor index will write, one per bucket a piece reaches (offsets: per piece
// of the index, n_pieces + 1, in scratch).
int bucket_pieces_count(mdb_ctx *ctx, const DevSegments &s, const BucketRequest &r, const unsigned long long *piece_base,
                        const MvIndex &index, const unsigned long long **offsets_out, unsigned long long *total);

// k_agg_bucket_check: *unsorted |= 1 if the m keys are not non-decreasing.
void bucket_keys_check(mdb_ctx *ctx, const unsigned long long *keys, uint64_t m, unsigned int *unsorted);

// The step between an operator's partials kernels and the fold of a slice (mdb_bucket_fold.hpp): the m keys checked,
// the two read-back words fetched (words[0]: the error bits the operator's kernels ORed, words[1]: the check's flag)
// and the stream synchronised. The caller makes its own message of *error.
int bucket_slice_check(mdb_ctx *ctx, const unsigned long long *keys, uint64_t m, unsigned int *words, unsigned int *error,
                       bool *unsorted);

// The sort path: the m keys in order (stable, rocPRIM's radix sort over key_bits bits) and the pair numbers alongside,
// both in scratch.
int bucket_keys_sort(mdb_ctx *ctx, unsigned long long *keys, uint64_t m, unsigned int key_bits,
                     const unsigned long long **sorted_keys, const uint32_t **order);

} // namespace mdb
