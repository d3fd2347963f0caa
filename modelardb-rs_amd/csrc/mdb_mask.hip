// mdb_mask.hip - row masks on segments: a predicate on one field column selects the rows of another
// (mdb_mask_filter_dev, mdb_mask_combine_dev, mdb_grid_batch_mask_dev, mdb_agg_batch_mask_dev, mdb_agg_batch_where,
// mdb_grid_batch_where_owned).
//
// What the reference computes with GridExec per field -> SortedJoinExec -> FilterExec (-> AggregateExec) for
// SELECT agg(a) FROM t WHERE b > c AND ...: every point of every named field is rebuilt, zipped by row position
// (query/sorted_join_exec.rs:278-310) and a BooleanArray per predicate decides the rows. Here the BooleanArray is made
// from the predicate field's segments and consumed by the target field's, and no point of either is materialised
// unless its segment has to be looked at point by point. Layout of a mask: mdb_mask.hpp.
//
//   rows and first rows   the range grid's prepass (grid_range_plan: every error the range calls report) gives the rows
//                         of each segment, an exclusive scan (mdb_scan.hpp) each segment's first row. Producer and
//                         consumers share this step: two batches line up when row r is the same data point in both.
//   k_mask_classify       producer, 1 lane / segment: classify_segment (mdb_filter_points.hpp) - none / one interval
//                         of model points / per point. An interval is a run of ones; the wave then writes the runs of
//                         its 64 segments as one list of 8-byte words, a word per lane and round: whole words with
//                         plain stores, the two end words of a run with an integer atomicOr (shared with neighbours).
//   k_mask_points_set     producer, per-point segments (MacaqueV, residual tails, irregular timestamps, NaN ends):
//                         gathered and rebuilt by the range grid in bounded slices exactly as the filtered grid does;
//                         one wave per segment, the __ballot of the predicate becomes mask bits (atomicOr of the two
//                         words the 64 rows reach into). Integer ORs commute: the mask does not depend on the order.
//   k_mask_combine        AND / OR / XOR / ANDNOT / NOT word by word, the tail of the last word cleared, the set
//                         bits counted (integer atomics on LDS and one counter).
//   k_mask_plan_rows      consumer (grid), 1 lane / segment: the segment's selected rows (popcount of its bit range:
//                         rows_per_segment), those among its model rows, and whether its other rows hold a set bit at
//                         all (only then is it rebuilt). Scan -> output offsets, one read-back sizes the output.
//   k_mask_write_runs     1 wave / segment: the selected model points start + k * delta, compacted 64 rows at a time
//                         with __popcll of the mask window (an all-zero window is skipped).
//   k_mask_points_write   the selected rows of the rebuilt slices, compacted with ballots as k_filter_points_write does
//                         (both, and k_mask_points_set, are slice_walk of mdb_filter_points.hpp with their own test
//                         and sink).
//   k_agg_mask            (mdb_agg.hip) the masked aggregates: k_agg_filter's loop and fixed reduction tree with the
//                         selector SegmentRows of mdb_mask.hpp in segment_range.
// All writes are ordinary vector stores; the only atomics are integer ones.
#include "mdb_filter_points.hpp"
#include "mdb_host_side.hpp"
#include "mdb_mask.hpp"
#include "mdb_scan.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace mdb {

constexpr int MASK_THREADS = 256;
static_assert(MASK_THREADS == FILTER_THREADS, "slice_walk's waves are counted in FILTER_THREADS");

// Adds `local` of every thread of the block to *counter: LDS first, then one integer atomic per block.
__device__ __forceinline__ void block_count_add(unsigned long long local, unsigned long long *lds,
                                                unsigned long long *__restrict__ counter) {
    if (threadIdx.x == 0) *lds = 0;
    __syncthreads();
    if (local) atomicAdd(lds, local);
    __syncthreads();
    if (threadIdx.x == 0 && *lds) atomicAdd(counter, *lds);
}

// Producer. per_point[i] as classify_segment's `tested`; the interval of segment i becomes the ones of rows
// first_row[i] + run_first .. + n - 1 of `mask` (cleared before the launch).
__global__ __launch_bounds__(MASK_THREADS) void k_mask_classify(DevSegments s, int64_t t_lo, int64_t t_hi, ValueKeys keys,
                                                                const unsigned long long *__restrict__ first_row,
                                                                unsigned long long *__restrict__ mask, uint64_t n_rows,
                                                                uint32_t *__restrict__ per_point) {
    const uint64_t i = (uint64_t)blockIdx.x * MASK_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & (MDB_WAVE - 1);
    uint64_t run_row = 0;
    uint32_t run_n = 0;
    if (i < s.n) {
        FilterRun r;
        uint32_t tested = 0, run_first = 0;
        classify_segment(s, i, t_lo, t_hi, keys, &r, &tested, &run_first);
        per_point[i] = tested;
        run_row = first_row[i] + run_first;
        // (a run is part of its segment's rows, which end below n_rows; no word beyond the mask is ever written)
        run_n = run_row < n_rows ? (uint32_t)min((uint64_t)r.n, n_rows - run_row) : 0u;
    }
    // The runs of the wave's 64 segments as ONE list of words, a word per lane and round: the lane finds the run its
    // word belongs to in the prefix sums of the runs' word counts (LDS, a search of 6 steps), so every lane stores in
    // every round however short the runs are.
    __shared__ uint64_t lds_row[MASK_THREADS];
    __shared__ uint32_t lds_n[MASK_THREADS], lds_before[MASK_THREADS];
    const uint32_t wave_base = threadIdx.x & ~(uint32_t)(MDB_WAVE - 1);
    const uint32_t n_words = run_n != 0 ? (uint32_t)(((run_row + run_n - 1) >> 6) - (run_row >> 6)) + 1u : 0u;
    uint32_t through = n_words; // inclusive prefix sum over the lanes
#pragma unroll
    for (int delta = 1; delta < MDB_WAVE; delta <<= 1) {
        const uint32_t below = __shfl_up(through, delta, MDB_WAVE);
        if ((int)lane >= delta) through += below;
    }
    const uint32_t total = __shfl(through, MDB_WAVE - 1, MDB_WAVE);
    lds_row[threadIdx.x] = run_row;
    lds_n[threadIdx.x] = run_n;
    lds_before[threadIdx.x] = through - n_words;
    __syncthreads();
    for (uint32_t t = lane; t < total; t += MDB_WAVE) {
        // the last lane whose words begin at or before t (lanes without a run share their successor's beginning)
        uint32_t lo = 0, hi = MDB_WAVE;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (lds_before[wave_base + mid] <= t) lo = mid;
            else hi = mid;
        }
        const uint64_t a = lds_row[wave_base + lo];
        const uint64_t e = a + lds_n[wave_base + lo] - 1; // the last row of the run
        const uint64_t w_first = a >> 6, w_last = e >> 6;
        const uint64_t w = w_first + (t - lds_before[wave_base + lo]);
        unsigned long long bits = ~0ull;
        if (w == w_first) bits &= ~0ull << (a & 63);
        if (w == w_last) bits &= ~0ull >> (63 - (e & 63));
        if (bits == ~0ull) mask[w] = bits; // (all 64 rows are this run's: nobody else writes the word)
        else atomicOr(&mask[w], bits);
    }
}

// Producer, the per-point segments of a slice (slice_walk, mdb_filter_points.hpp): the rows whose value passes become
// ones - lane 0 ORs the round's ballot into the two words its 64 rows reach into.
__global__ __launch_bounds__(MASK_THREADS) void k_mask_points_set(const float *__restrict__ slice_val,
                                                                  const unsigned long long *__restrict__ first,
                                                                  uint64_t n_slice, uint64_t j0, Gathered g, ValueKeys keys,
                                                                  const unsigned long long *__restrict__ first_row,
                                                                  unsigned long long *__restrict__ mask, uint64_t n_words) {
    slice_walk(first, n_slice, j0, g, [&](uint32_t, uint64_t) { return [&](uint64_t row) { return keys.pass(slice_val[row]); }; },
               [&](uint32_t origin, uint64_t begin) {
                   const uint64_t segment_row = first_row[origin];
                   return [&, segment_row, begin](uint64_t row0, uint64_t row, bool, unsigned long long bits, uint64_t) {
                       if (row != row0 || bits == 0) return; // (lane 0)
                       const uint64_t r = segment_row + (row0 - begin);
                       const uint32_t shift = (uint32_t)(r & 63);
                       const uint64_t w = r >> 6; // (below n_words, as every row of a segment is: never a word beyond the mask)
                       if (w < n_words) atomicOr(&mask[w], bits << shift);
                       if (shift != 0 && (bits >> (64 - shift)) != 0 && w + 1 < n_words) atomicOr(&mask[w + 1], bits >> (64 - shift));
                   };
               },
               [](uint32_t, uint64_t) {});
}

__global__ __launch_bounds__(MASK_THREADS) void k_mask_count(const unsigned long long *__restrict__ mask, uint64_t n_words,
                                                             unsigned long long *__restrict__ counter) {
    __shared__ unsigned long long lds;
    unsigned long long local = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * MASK_THREADS + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * MASK_THREADS)
        local += (unsigned long long)__popcll(mask[w]);
    block_count_add(local, &lds, counter);
}

// out = a op b word by word (every thread reads its words before it writes: out may be a or b); `tail`: the valid
// bits of the last word.
__global__ __launch_bounds__(MASK_THREADS) void k_mask_combine(uint32_t op, const unsigned long long *a,
                                                               const unsigned long long *b, unsigned long long *out,
                                                               uint64_t n_words, unsigned long long tail,
                                                               unsigned long long *__restrict__ counter) {
    __shared__ unsigned long long lds;
    unsigned long long local = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * MASK_THREADS + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * MASK_THREADS) {
        const unsigned long long x = a[w];
        const unsigned long long y = op == MDB_MASK_NOT ? 0ull : b[w];
        unsigned long long z;
        switch (op) {
        case MDB_MASK_AND: z = x & y; break;
        case MDB_MASK_OR: z = x | y; break;
        case MDB_MASK_XOR: z = x ^ y; break;
        case MDB_MASK_ANDNOT: z = x & ~y; break;
        default: z = ~x; break;
        }
        if (w == n_words - 1) z &= tail;
        out[w] = z;
        local += (unsigned long long)__popcll(z);
    }
    if (counter) block_count_add(local, &lds, counter);
}

// Consumer (grid). Segment i under [t_lo, t_hi] with every value passing: its model rows as a run (runs[i]), the
// set bits among all its rows (counts[i]) and among the run's (model_sel[i]), and per_point[i] as classify_segment's
// `tested` - 0 as well when none of the rows to be looked at one by one is selected.
__global__ __launch_bounds__(MASK_THREADS) void k_mask_plan_rows(DevSegments s, int64_t t_lo, int64_t t_hi,
                                                                 const uint32_t *__restrict__ rows,
                                                                 const unsigned long long *__restrict__ first_row,
                                                                 RowBits bits, FilterRun *__restrict__ runs,
                                                                 uint32_t *__restrict__ per_point,
                                                                 uint32_t *__restrict__ counts,
                                                                 uint32_t *__restrict__ model_sel) {
    const uint64_t i = (uint64_t)blockIdx.x * MASK_THREADS + threadIdx.x;
    if (i >= s.n) return;
    FilterRun r;
    uint32_t tested = 0, run_first = 0;
    classify_segment(s, i, t_lo, t_hi, ValueKeys{INT32_MIN, INT32_MAX}, &r, &tested, &run_first);
    const uint64_t row = first_row[i];
    const uint32_t n_rows = rows[i];
    if (r.n > n_rows) r.n = n_rows; // (never: the run is part of the segment's rows)
    const uint32_t all = bits.count(row, n_rows);
    const uint32_t model = bits.count(row, r.n);
    if (all == model) tested = 0;
    runs[i] = r;
    per_point[i] = tested;
    counts[i] = all;
    model_sel[i] = model;
}

// One wave per segment: the selected ones of its run's points, from offsets[i] on. out_ts may be nullptr.
__global__ __launch_bounds__(MASK_THREADS) void k_mask_write_runs(const FilterRun *__restrict__ runs, uint64_t n,
                                                                  const unsigned long long *__restrict__ first_row,
                                                                  RowBits bits, const uint32_t *__restrict__ model_sel,
                                                                  const unsigned long long *__restrict__ offsets,
                                                                  int64_t *__restrict__ out_ts, float *__restrict__ out_val) {
    const uint32_t lane = threadIdx.x & (MDB_WAVE - 1);
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint64_t waves = (uint64_t)gridDim.x * (MASK_THREADS / MDB_WAVE);
    for (uint64_t i = (uint64_t)blockIdx.x * (MASK_THREADS / MDB_WAVE) + threadIdx.x / MDB_WAVE; i < n; i += waves) {
        if (model_sel[i] == 0) continue;
        const FilterRun r = runs[i];
        const uint64_t base = offsets[i], row = first_row[i];
        uint64_t kept = 0;
        for (uint32_t k0 = 0; k0 < r.n; k0 += MDB_WAVE) {
            unsigned long long w = bits.window(row + k0);
            if (r.n - k0 < MDB_WAVE) w &= (1ull << (r.n - k0)) - 1ull;
            if (w == 0) continue;
            if ((w >> lane) & 1ull) {
                const uint64_t at = base + kept + (uint64_t)__popcll(w & below);
                int64_t t;
                float v;
                run_point(r, k0 + lane, &t, &v);
                if (out_ts) out_ts[at] = t;
                out_val[at] = v;
            }
            kept += (uint64_t)__popcll(w);
        }
    }
}

// The per-point segments of a slice (slice_walk): their selected rows behind the first skip ones, in order, behind the
// segment's selected model rows. out_ts may be nullptr.
__global__ __launch_bounds__(MASK_THREADS) void k_mask_points_write(
    const int64_t *__restrict__ slice_ts, const float *__restrict__ slice_val, const unsigned long long *__restrict__ first,
    uint64_t n_slice, uint64_t j0, Gathered g, const unsigned long long *__restrict__ first_row, RowBits bits,
    const uint32_t *__restrict__ model_sel, const unsigned long long *__restrict__ offsets, int64_t *__restrict__ out_ts,
    float *__restrict__ out_val) {
    slice_walk(first, n_slice, j0, g,
               [&](uint32_t origin, uint64_t begin) {
                   const uint64_t segment_row = first_row[origin];
                   return [&, segment_row, begin](uint64_t row) { return bits.test(segment_row + (row - begin)); };
               },
               [&](uint32_t origin, uint64_t) {
                   const uint64_t out = offsets[origin] + model_sel[origin];
                   return [&, out](uint64_t, uint64_t row, bool pass, unsigned long long ballot, uint64_t kept) {
                       slice_write_row(out + kept, row, pass, ballot, slice_ts, slice_val, out_ts, out_val);
                   };
               },
               [](uint32_t, uint64_t) {});
}

namespace {

uint64_t words_of(uint64_t n_rows) { return n_rows / 64 + (n_rows % 64 != 0 ? 1 : 0); }

// The per-segment arrays of one call (SCRATCH_MASK_SEGMENTS).
struct MaskScratch {
    uint32_t *rows = nullptr;                 // rows of the range grid
    unsigned long long *first_row = nullptr;  // their exclusive scan (n + 1)
    uint32_t *per_point = nullptr;
    uint32_t *counts = nullptr;               // selected rows
    uint32_t *model_sel = nullptr;            // ... among the run's
    FilterRun *runs = nullptr;
    unsigned long long *position = nullptr;   // (n + 1) the gather's scan
    unsigned long long *offsets = nullptr;    // (n + 1) output offsets
    unsigned long long *block_sums = nullptr;
    unsigned long long *words = nullptr;      // 4 words: rows by type, a counter
};

int mask_scratch(mdb_ctx *ctx, uint64_t n, MaskScratch *m) {
    const uint64_t b4 = align_up(n * 4, 256), b8 = align_up((n + 1) * 8, 256), runs = align_up(n * sizeof(FilterRun), 256);
    const uint64_t sums = align_up(scan_block_sums_bytes(n), 256);
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_MASK_SEGMENTS, 4 * b4 + 3 * b8 + runs + sums + 256, &p)) return 1;
    Carver scratch(p);
    m->runs = scratch.take<FilterRun>(n);
    m->first_row = scratch.take<unsigned long long>(n + 1);
    m->position = scratch.take<unsigned long long>(n + 1);
    m->offsets = scratch.take<unsigned long long>(n + 1);
    m->block_sums = scratch.take<unsigned long long>(scan_block_sums_bytes(n) / 8);
    m->words = scratch.take<unsigned long long>(4);
    m->rows = scratch.take<uint32_t>(n);
    m->per_point = scratch.take<uint32_t>(n);
    m->counts = scratch.take<uint32_t>(n);
    m->model_sel = scratch.take<uint32_t>(n);
    return 0;
}

// The rows of the batch under [t_lo, t_hi]: the range grid's prepass (its errors, its segment counters), rows per
// segment, and each segment's first row.
int rows_plan(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, MaskScratch *m, uint64_t *total,
              mdb_grid_metrics *metrics) {
    if (in->n > 0xffffffffull) return fail("Too many segments for one masked call.");
    if (mask_scratch(ctx, in->n, m)) return 1;
    if (grid_range_plan(ctx, in, t_lo, t_hi, total, metrics, m->rows)) return 1;
    if (in->n == 0) return 0;
    return device_exclusive_scan(ctx, ItemsOf<uint32_t>{m->rows}, in->n, m->first_row, m->block_sums, "k_mask_scan");
}

int count_bits(mdb_ctx *ctx, const unsigned long long *mask, uint64_t n_words, unsigned long long *counter, uint64_t *n_set) {
    unsigned long long set = 0;
    if (n_words > 0) {
        MDB_HIP_CHECK(hipMemsetAsync(counter, 0, 8, ctx->stream));
        {
            LaunchTimer timer(ctx, "k_mask_count");
            const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_words + MASK_THREADS - 1) / MASK_THREADS, 2048);
            hipLaunchKernelGGL(k_mask_count, dim3(blocks), dim3(MASK_THREADS), 0, ctx->stream, mask, n_words, counter);
        }
        MDB_HIP_CHECK(hipMemcpyAsync(&set, counter, 8, hipMemcpyDeviceToHost, ctx->stream));
        MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    *n_set = set;
    return 0;
}

// The mask of (keys, [t_lo, t_hi]) over a batch in HBM into `mask` (cap_words words). expected_rows (may be nullptr):
// the number of rows the batch must have under the range (the host forms: the target's).
int mask_filter_locked(mdb_ctx *ctx, const mdb_segments *in, const ValueKeys &keys, int64_t t_lo, int64_t t_hi,
                       unsigned long long *mask, uint64_t cap_words, const uint64_t *expected_rows, uint64_t *n_rows,
                       uint64_t *n_set) {
    MaskScratch m;
    uint64_t total = 0;
    if (rows_plan(ctx, in, t_lo, t_hi, &m, &total, nullptr)) return 1;
    if (expected_rows && total != *expected_rows)
        return fail("A predicate field has " + std::to_string(total) + " rows under the time range but the target has " +
                    std::to_string(*expected_rows) + ": the batches do not line up.");
    const uint64_t n_words = words_of(total);
    if (n_words > cap_words)
        return fail("Mask buffer too small: " + std::to_string(total) + " rows need " + std::to_string(n_words) +
                    " words but cap_words is " + std::to_string(cap_words) + ".");
    if (n_words > 0 && !mask) return fail("mask must not be NULL.");
    uint64_t set = 0;
    if (n_words > 0) {
        const uint64_t n = in->n;
        MDB_HIP_CHECK(hipMemsetAsync(mask, 0, n_words * 8, ctx->stream));
        {
            LaunchTimer timer(ctx, "k_mask_classify");
            hipLaunchKernelGGL(k_mask_classify, dim3((uint32_t)((n + MASK_THREADS - 1) / MASK_THREADS)), dim3(MASK_THREADS), 0,
                               ctx->stream, to_dev(in), t_lo, t_hi, keys, m.first_row, mask, total, m.per_point);
        }
        FilterPass f;
        f.in = in;
        f.t_lo = t_lo;
        f.t_hi = t_hi;
        f.keys = keys;
        if (filter_tested_slices(ctx, f, m.per_point, m.position, m.block_sums, [&](uint64_t j0, uint64_t n_slice) {
                LaunchTimer timer(ctx, "k_mask_points_set");
                hipLaunchKernelGGL(k_mask_points_set, dim3(slice_walk_blocks(n_slice, 8192)), dim3(MASK_THREADS), 0, ctx->stream,
                                   f.slice_val, f.slice_first, n_slice, j0, f.g, keys, m.first_row, mask, n_words);
            }))
            return 1;
        if (n_set && count_bits(ctx, mask, n_words, m.words + 3, &set)) return 1;
    }
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    *n_rows = total;
    if (n_set) *n_set = set;
    return 0;
}

int mask_combine_locked(mdb_ctx *ctx, uint32_t op, const unsigned long long *a, const unsigned long long *b,
                        unsigned long long *out, uint64_t n_rows, uint64_t *n_set) {
    const uint64_t n_words = words_of(n_rows);
    unsigned long long set = 0;
    if (n_words > 0) {
        unsigned long long *counter = nullptr;
        if (n_set) {
            void *p = nullptr;
            if (scratch_reserve(ctx, SCRATCH_MASK_SEGMENTS, 256, &p)) return 1;
            counter = static_cast<unsigned long long *>(p);
            MDB_HIP_CHECK(hipMemsetAsync(counter, 0, 8, ctx->stream));
        }
        const unsigned long long tail = n_rows % 64 != 0 ? (1ull << (n_rows % 64)) - 1ull : ~0ull;
        {
            LaunchTimer timer(ctx, "k_mask_combine");
            const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_words + MASK_THREADS - 1) / MASK_THREADS, 2048);
            hipLaunchKernelGGL(k_mask_combine, dim3(blocks), dim3(MASK_THREADS), 0, ctx->stream, op, a, b, out, n_words, tail,
                               counter);
        }
        if (n_set) MDB_HIP_CHECK(hipMemcpyAsync(&set, counter, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (n_set) *n_set = set;
    return 0;
}

// One masked grid call over a batch in HBM: what the count leaves for the write.
struct MaskGridPass {
    const mdb_segments *in = nullptr;
    int64_t t_lo = 0, t_hi = 0;
    RowBits bits{nullptr, 0};
    MaskScratch m;
    uint64_t total = 0; // rows produced
    mdb_grid_metrics metrics{};
};

int row_count_mismatch(uint64_t batch_rows, uint64_t mask_rows) {
    return fail("The batch has " + std::to_string(batch_rows) + " rows under the time range but the mask has " +
                std::to_string(mask_rows) + " rows.");
}

// Pass 1: rows and first rows, the selected rows of every segment, their scan. Sets g.total and g.metrics.
int mask_grid_count(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const unsigned long long *mask,
                    uint64_t n_rows, MaskGridPass &g) {
    g.in = in;
    g.t_lo = t_lo;
    g.t_hi = t_hi;
    uint64_t batch_rows = 0;
    if (rows_plan(ctx, in, t_lo, t_hi, &g.m, &batch_rows, &g.metrics)) return 1;
    if (batch_rows != n_rows) return row_count_mismatch(batch_rows, n_rows);
    if (n_rows > 0 && !mask) return fail("mask must not be NULL.");
    g.bits = RowBits{mask, words_of(n_rows)};
    g.metrics.rows_created = 0;
    for (int k = 0; k < 3; k++) g.metrics.rows_created_by_model_type[k] = 0;
    const uint64_t n = in->n;
    if (n == 0) return 0;
    {
        LaunchTimer timer(ctx, "k_mask_plan_rows");
        hipLaunchKernelGGL(k_mask_plan_rows, dim3((uint32_t)((n + MASK_THREADS - 1) / MASK_THREADS)), dim3(MASK_THREADS), 0,
                           ctx->stream, to_dev(in), t_lo, t_hi, g.m.rows, g.m.first_row, g.bits, g.m.runs, g.m.per_point,
                           g.m.counts, g.m.model_sel);
    }
    return filter_count_done(ctx, in, g.m.counts, g.m.offsets, g.m.block_sums, g.m.words, "k_mask_scan", &g.total, &g.metrics);
}

// Pass 2: the rows into out_ts (may be nullptr) / out_val, rows per segment into out_rows (may be nullptr).
int mask_grid_write(mdb_ctx *ctx, MaskGridPass &g, int64_t *out_ts, float *out_val, uint32_t *out_rows) {
    const uint64_t n = g.in->n;
    if (n == 0) return 0;
    if (g.total > 0) {
        {
            LaunchTimer timer(ctx, "k_mask_write_runs");
            hipLaunchKernelGGL(k_mask_write_runs, dim3(slice_walk_blocks(n, 16384)), dim3(MASK_THREADS), 0, ctx->stream, g.m.runs, n,
                               g.m.first_row, g.bits, g.m.model_sel, g.m.offsets, out_ts, out_val);
        }
        FilterPass f;
        f.in = g.in;
        f.t_lo = g.t_lo;
        f.t_hi = g.t_hi;
        if (filter_tested_slices(ctx, f, g.m.per_point, g.m.position, g.m.block_sums, [&](uint64_t j0, uint64_t n_slice) {
                LaunchTimer timer(ctx, "k_mask_points_write");
                hipLaunchKernelGGL(k_mask_points_write, dim3(slice_walk_blocks(n_slice, 8192)), dim3(MASK_THREADS), 0, ctx->stream,
                                   f.slice_ts, f.slice_val, f.slice_first, n_slice, j0, f.g, g.m.first_row, g.bits,
                                   g.m.model_sel, g.m.offsets, out_ts, out_val);
            }))
            return 1;
    }
    if (out_rows) MDB_HIP_CHECK(hipMemcpyAsync(out_rows, g.m.counts, n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int agg_mask_locked(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const unsigned long long *mask,
                    uint64_t n_rows, uint32_t which_mask, mdb_agg_state *inout) {
    MaskScratch m;
    uint64_t batch_rows = 0;
    if (rows_plan(ctx, in, t_lo, t_hi, &m, &batch_rows, nullptr)) return 1;
    if (batch_rows != n_rows) return row_count_mismatch(batch_rows, n_rows);
    if (n_rows == 0) return 0;
    if (!mask) return fail("mask must not be NULL.");
    return agg_mask_run(ctx, in, t_lo, t_hi, m.first_row, mask, words_of(n_rows), which_mask, inout);
}

// ---- the host forms: WHERE p_0(field_0) AND p_1(field_1) ... over host batches ---------------------------------

// The batches of one call in HBM: every distinct host batch once (the target may be one of the predicate fields).
struct Uploads {
    std::vector<std::pair<const mdb_segments *, mdb_segments_owned *>> list;
    ~Uploads() {
        for (auto &entry : list) mdb_segments_free(entry.second);
    }
    int get(mdb_ctx *ctx, const mdb_segments *host, const mdb_segments **dev) {
        for (auto &entry : list)
            if (entry.first == host) {
                *dev = &entry.second->seg;
                return 0;
            }
        // (not into the context's upload scratch: that holds one batch at a time)
        mdb_segments_owned *owned = nullptr;
        if (upload_segments_locked(ctx, host, false, &owned)) return 1;
        list.push_back({host, owned});
        *dev = &owned->seg;
        return 0;
    }
};

struct Where {
    std::vector<ValueKeys> keys;
    int64_t t_lo = INT64_MIN, t_hi = INT64_MAX; // the intersection of the filters' time ranges
};

int where_check(const mdb_segments *const *pred_fields, const mdb_value_filter *filters, uint32_t n_preds, Where *w) {
    if (n_preds > 0 && (!pred_fields || !filters)) return fail("pred_fields and filters must not be NULL.");
    w->keys.resize(n_preds);
    for (uint32_t k = 0; k < n_preds; k++) {
        if (!pred_fields[k]) return fail("A batch of pred_fields is NULL.");
        if (value_keys_fold(&filters[k], &w->keys[k])) return 1;
        w->t_lo = std::max(w->t_lo, filters[k].t_lo);
        w->t_hi = std::min(w->t_hi, filters[k].t_hi);
    }
    return 0;
}

// The conjunction's mask over the target's rows under [w.t_lo, w.t_hi], in the context's scratch.
int where_mask(mdb_ctx *ctx, const mdb_segments *const *pred_fields, uint32_t n_preds, const Where &w, Uploads &uploads,
               const mdb_segments *target_dev, unsigned long long **mask, uint64_t *n_rows) {
    uint64_t rows = 0;
    if (grid_range_plan(ctx, target_dev, w.t_lo, w.t_hi, &rows, nullptr, nullptr)) return 1;
    const uint64_t n_words = words_of(rows), bytes = align_up(n_words * 8, 256);
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_MASK_WORDS, 2 * bytes, &p)) return 1;
    unsigned long long *all = static_cast<unsigned long long *>(p);
    unsigned long long *one = reinterpret_cast<unsigned long long *>(static_cast<uint8_t *>(p) + bytes);
    if (n_preds == 0 && n_words > 0) { // every row: NOT of the empty mask (clears the tail)
        MDB_HIP_CHECK(hipMemsetAsync(all, 0, n_words * 8, ctx->stream));
        if (mask_combine_locked(ctx, MDB_MASK_NOT, all, nullptr, all, rows, nullptr)) return 1;
    }
    for (uint32_t k = 0; k < n_preds; k++) {
        const mdb_segments *dev = nullptr;
        if (uploads.get(ctx, pred_fields[k], &dev)) return 1;
        uint64_t field_rows = 0;
        if (mask_filter_locked(ctx, dev, w.keys[k], w.t_lo, w.t_hi, k == 0 ? all : one, n_words, &rows, &field_rows, nullptr))
            return 1;
        if (k > 0 && mask_combine_locked(ctx, MDB_MASK_AND, all, one, all, rows, nullptr)) return 1;
    }
    *mask = all;
    *n_rows = rows;
    return 0;
}

} // namespace

} // namespace mdb

using namespace mdb;

extern "C" {

int mdb_mask_filter_dev(mdb_ctx *ctx, const mdb_segments *in, const mdb_value_filter *filter, uint64_t *mask,
                        uint64_t cap_words, uint64_t *n_rows, uint64_t *n_set) {
    if (!ctx || !in || !filter || !n_rows) return fail("ctx, in, filter and n_rows must not be NULL.");
    ValueKeys keys;
    if (value_keys_fold(filter, &keys)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    uint64_t rows = 0, set = 0;
    if (mask_filter_locked(ctx, in, keys, filter->t_lo, filter->t_hi, reinterpret_cast<unsigned long long *>(mask), cap_words,
                           nullptr, &rows, n_set ? &set : nullptr))
        return 1;
    *n_rows = rows;
    if (n_set) *n_set = set;
    return 0;
}

int mdb_mask_combine_dev(mdb_ctx *ctx, uint32_t op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n_rows,
                         uint64_t *n_set) {
    if (!ctx) return fail("ctx must not be NULL.");
    if (op != MDB_MASK_AND && op != MDB_MASK_OR && op != MDB_MASK_XOR && op != MDB_MASK_ANDNOT && op != MDB_MASK_NOT)
        return fail("Unknown mask operation " + std::to_string(op) + ".");
    if (op == MDB_MASK_NOT && b) return fail("b must be NULL for MDB_MASK_NOT.");
    if (n_rows > 0 && (!a || !out || (op != MDB_MASK_NOT && !b))) return fail("a, b and out must not be NULL.");
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return mask_combine_locked(ctx, op, reinterpret_cast<const unsigned long long *>(a),
                               reinterpret_cast<const unsigned long long *>(b), reinterpret_cast<unsigned long long *>(out),
                               n_rows, n_set);
}

int mdb_grid_batch_mask_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const uint64_t *mask,
                            uint64_t n_rows, int64_t *out_ts, float *out_val, uint32_t *out_rows_per_segment, uint64_t cap,
                            uint64_t *n_out, mdb_grid_metrics *metrics) {
    if (!ctx || !in) return fail("ctx and in must not be NULL.");
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    MaskGridPass g;
    if (mask_grid_count(ctx, in, t_lo, t_hi, reinterpret_cast<const unsigned long long *>(mask), n_rows, g)) return 1;
    if (g.total > cap)
        return fail("Output buffers too small: " + std::to_string(g.total) + " data points but capacity " +
                    std::to_string(cap) + ".");
    if (g.total > 0 && !out_val) return fail("out_val must not be NULL.");
    if (mask_grid_write(ctx, g, out_ts, out_val, out_rows_per_segment)) return 1;
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (n_out) *n_out = g.total;
    if (metrics) *metrics = g.metrics;
    return 0;
}

int mdb_agg_batch_mask_dev(mdb_ctx *ctx, const mdb_segments *in, int64_t t_lo, int64_t t_hi, const uint64_t *mask,
                           uint64_t n_rows, uint32_t which_mask, mdb_agg_state *inout) {
    if (!ctx || !in || !inout) return fail("ctx, in and inout must not be NULL.");
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return agg_mask_locked(ctx, in, t_lo, t_hi, reinterpret_cast<const unsigned long long *>(mask), n_rows, which_mask, inout);
}

int mdb_agg_batch_where(mdb_ctx *ctx, const mdb_segments *const *pred_fields, const mdb_value_filter *filters,
                        uint32_t n_preds, const mdb_segments *target, uint32_t which_mask, mdb_agg_state *inout) {
    if (!ctx || !target || !inout) return fail("ctx, target and inout must not be NULL.");
    Where w;
    if (where_check(pred_fields, filters, n_preds, &w)) return 1;
    if (n_preds == 0) return mdb_agg_batch_range(ctx, target, INT64_MIN, INT64_MAX, which_mask, inout);
    if (w.t_lo > w.t_hi) return 0; // (an empty intersection of the time ranges selects nothing)
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    Uploads uploads;
    const mdb_segments *target_dev = nullptr;
    if (uploads.get(ctx, target, &target_dev)) return 1;
    unsigned long long *mask = nullptr;
    uint64_t n_rows = 0;
    if (where_mask(ctx, pred_fields, n_preds, w, uploads, target_dev, &mask, &n_rows)) return 1;
    return agg_mask_locked(ctx, target_dev, w.t_lo, w.t_hi, mask, n_rows, which_mask, inout);
}

int mdb_grid_batch_where_owned(mdb_ctx *ctx, const mdb_segments *const *pred_fields, const mdb_value_filter *filters,
                               uint32_t n_preds, const mdb_segments *target, uint32_t flags, uint64_t reserve_front,
                               mdb_grid_result **out) {
    if (!ctx || !target || !out) return fail("ctx, target and out must not be NULL.");
    if ((flags & ~MDB_GRID_VALUES_ONLY) != 0) return fail("Unknown flag bits (MDB_GRID_VALUES_ONLY or 0).");
    Where w;
    if (where_check(pred_fields, filters, n_preds, &w)) return 1;
    const bool values_only = (flags & MDB_GRID_VALUES_ONLY) != 0;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    if (w.t_lo > w.t_hi) // an empty intersection of the time ranges selects nothing
        return owned_result(ctx, nullptr, result_layout(reserve_front, 0, target->n, values_only), mdb_grid_metrics{}, out);
    Uploads uploads;
    const mdb_segments *target_dev = nullptr;
    if (uploads.get(ctx, target, &target_dev)) return 1;
    unsigned long long *mask = nullptr;
    uint64_t n_rows = 0;
    if (where_mask(ctx, pred_fields, n_preds, w, uploads, target_dev, &mask, &n_rows)) return 1;
    MaskGridPass g;
    if (mask_grid_count(ctx, target_dev, w.t_lo, w.t_hi, mask, n_rows, g)) return 1;
    const ResultLayout layout = result_layout(reserve_front, g.total, target->n, values_only);
    void *stage = nullptr;
    if (scratch_reserve(ctx, SCRATCH_STAGE_DEV, layout.bytes(), &stage)) return 1;
    if (target->n == 0) MDB_HIP_CHECK(hipMemsetAsync(layout.rows(stage), 0, layout.rows_bytes, ctx->stream));
    if (mask_grid_write(ctx, g, layout.timestamps(stage), layout.values(stage), layout.rows(stage))) return 1;
    return owned_result(ctx, stage, layout, g.metrics, out);
}

} // extern "C"
