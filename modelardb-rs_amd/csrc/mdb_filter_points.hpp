// mdb_filter_points.hpp - what the filtered grid (mdb_filter.hip) and the row masks (mdb_mask.hip) share: the three
// classes a time-clipped segment falls into under a value predicate (classify_segment), the k-th point of an interval
// (run_point), and the segments whose points have to be looked at one by one, gathered into a batch of their own and
// rebuilt by the range grid in bounded slices (FilterPass, filter_tested_slices) whose rows one wave per segment walks
// 64 at a time (slice_walk); then what a count leaves for its write (filter_count_done).
#pragma once

#include "mdb_filter.hpp"

#include <utility>
#include <vector>

namespace mdb {

constexpr int FILTER_THREADS = 256;

// An interval segment's passing model points: n points from timestamp `start` on, `delta` apart.
struct FilterRun {
    int64_t start;
    int64_t delta;
    double slope;
    double intercept;
    float value;
    uint32_t type;
    uint32_t n;
    uint32_t pad;
};
static_assert(sizeof(FilterRun) == 48, "48 B per segment");

// The k-th point of a run.
__device__ __forceinline__ void run_point(const FilterRun &r, uint32_t k, int64_t *t, float *v) {
    const int64_t time = r.start + (int64_t)((uint64_t)k * (uint64_t)r.delta);
    *t = time;
    *v = r.type == MDB_SWING_ID ? (float)(r.slope * (double)time + r.intercept) : r.value;
}

// Segment i under [t_lo, t_hi] and `keys`. *run: the passing model points of its interval (n == 0: none).
// *tested: 0 - no point of the segment is tested one by one; 1 + m - its rows in the range grid are tested from the
// (m + 1)-th on (m: the model rows the interval has already decided). *run_first: the row of the segment (counted
// from its first row in the range grid) the interval begins at.
// (the range grid takes no point of a segment outside the range; its errors are grid_range_plan's to report)
__device__ __forceinline__ void classify_segment(const DevSegments &s, uint64_t i, int64_t t_lo, int64_t t_hi,
                                                 const ValueKeys &keys, FilterRun *run, uint32_t *tested,
                                                 uint32_t *run_first) {
    FilterRun r{0, 0, 0.0, 0.0, 0.0f, 0u, 0u, 0u};
    *tested = 0;
    *run_first = 0;
    if (!(s.end_time[i] < t_lo || s.start_time[i] > t_hi)) {
        const SegInfo info = analyse_segment(s, i);
        const SegDesc &d = info.desc;
        const uint32_t type = d.flags & FLAG_TYPE_MASK;
        uint32_t k_lo = 0, k_hi = 0;
        if (info.error) {
        } else if (!(d.flags & FLAG_REGULAR) || type == MDB_MACAQUE_V_ID) {
            *tested = 1;
        } else if (regular_index_interval(d.start, d.delta, d.n_total, t_lo, t_hi, &k_lo, &k_hi)) {
            uint32_t model_rows = 0;
            bool whole = false;
            if (k_lo < d.n_model) {
                const uint32_t a = k_lo, b = min(k_hi, d.n_model - 1);
                model_rows = b - a + 1;
                uint32_t ra = a, rb = b;
                const int run_class = model_run(d, type, a, b, keys, &ra, &rb);
                if (run_class == RUN_POINTS) {
                    whole = true;
                } else if (run_class == RUN_INTERVAL) {
                    r.start = d.start + (int64_t)((uint64_t)ra * (uint64_t)d.delta);
                    r.delta = d.delta;
                    r.slope = d.slope;
                    r.intercept = d.intercept;
                    r.value = d.value;
                    r.type = type;
                    r.n = rb - ra + 1;
                    *run_first = ra - a;
                }
            }
            if (whole) *tested = 1;
            else if (d.n_total > d.n_model && k_hi >= d.n_model) *tested = 1 + model_rows;
        }
    }
    *run = r;
}

// The columns of the per-point segments, in segment order, with the same payload buffers.
struct Gathered {
    int8_t *type;
    int64_t *start;
    int64_t *end;
    float *min;
    float *max;
    uint4 *ts_views;
    uint4 *value_views;
    uint4 *residual_views;
    uint32_t *origin;    // the segment of the batch
    uint32_t *skip;      // rows of the range grid the interval has decided
    uint32_t *rows;      // rows of the range grid
};

// One wave per per-point segment of a slice (rows [first[j], first[j + 1]) of the slice's range grid, gathered
// segment j0 + j, segment `origin` of the batch): its rows behind the first skip ones, 64 at a time. Per segment,
// select_of(origin, begin) gives the test of a row and sink_of(origin, begin) what takes a round's outcome:
// selected(row) of every lane's row -> __ballot -> take(row0, row, pass, ballot, kept), kept: the rows selected in the
// rounds before. done(origin, kept) ends the segment.
template <typename SelectOf, typename SinkOf, typename Done>
__device__ __forceinline__ void slice_walk(const unsigned long long *__restrict__ first, uint64_t n_slice, uint64_t j0,
                                           const Gathered &g, SelectOf select_of, SinkOf sink_of, Done done) {
    const uint32_t lane = threadIdx.x & (MDB_WAVE - 1);
    const uint64_t waves = (uint64_t)gridDim.x * (FILTER_THREADS / MDB_WAVE);
    for (uint64_t j = (uint64_t)blockIdx.x * (FILTER_THREADS / MDB_WAVE) + threadIdx.x / MDB_WAVE; j < n_slice; j += waves) {
        const uint32_t origin = g.origin[j0 + j];
        const uint64_t begin = first[j], end = first[j + 1];
        const auto selected = select_of(origin, begin);
        const auto take = sink_of(origin, begin);
        uint64_t kept = 0;
        for (uint64_t row0 = begin + g.skip[j0 + j]; row0 < end; row0 += MDB_WAVE) {
            const uint64_t row = row0 + lane;
            const bool pass = row < end && selected(row);
            const unsigned long long ballot = __ballot(pass);
            take(row0, row, pass, ballot, kept);
            kept += (uint64_t)__popcll(ballot);
        }
        done(origin, kept);
    }
}
// (the sink of the two kernels that write: the selected rows, in order, from out[origin] on)
__device__ __forceinline__ void slice_write_row(uint64_t out, uint64_t row, bool pass, unsigned long long ballot,
                                                const int64_t *__restrict__ slice_ts, const float *__restrict__ slice_val,
                                                int64_t *__restrict__ out_ts, float *__restrict__ out_val) {
    if (!pass) return;
    const uint32_t lane = threadIdx.x & (MDB_WAVE - 1);
    const uint64_t at = out + (uint64_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (out_ts) out_ts[at] = slice_ts[row];
    out_val[at] = slice_val[row];
}
inline uint32_t slice_walk_blocks(uint64_t n_slice, uint32_t most) { // (launches of one wave per segment)
    const uint64_t per_block = FILTER_THREADS / MDB_WAVE;
    return (uint32_t)((n_slice + per_block - 1) / per_block < most ? (n_slice + per_block - 1) / per_block : most);
}

// One filtered grid call over a batch in HBM: what the count leaves for the write.
struct FilterPass {
    const mdb_segments *in = nullptr;
    int64_t t_lo = 0, t_hi = 0;
    ValueKeys keys{INT32_MAX, INT32_MIN};
    uint64_t total = 0;            // rows produced
    mdb_grid_metrics metrics{};
    FilterRun *runs = nullptr;
    uint32_t *counts = nullptr;    // rows per segment
    unsigned long long *offsets = nullptr;
    // the per-point segments
    uint64_t n_tested = 0;
    mdb_segments tested{};         // their batch (the gathered columns)
    Gathered g{};
    std::vector<std::pair<uint64_t, uint64_t>> slices; // [j0, j1) of the gathered segments
    uint64_t slice_cap = 0;
    int64_t *slice_ts = nullptr;
    float *slice_val = nullptr;
    uint32_t *slice_rows = nullptr;
    unsigned long long *slice_first = nullptr;
    unsigned long long *slice_block_sums = nullptr;
    bool kept = false;             // one slice, still in place from the count
};

// mdb_filter.hip (the lock held, the device set; f.in, f.t_lo and f.t_hi filled in):
// The segments with per_point[i] != 0 gathered into f.tested (f.n_tested of them; `position`, n + 1 words, and
// `block_sums` are the caller's scan scratch), cut into f.slices, the slice buffers reserved. One synchronisation.
int filter_gather_tested(mdb_ctx *ctx, FilterPass &f, const uint32_t *per_point, unsigned long long *position,
                         unsigned long long *block_sums);
// The range grid of gathered segments [j0, j1) into the slice buffers, and the first row of each (f.slice_first).
int filter_rebuild_slice(mdb_ctx *ctx, FilterPass &f, uint64_t j0, uint64_t j1);
// The per-point segments gathered (per_point nullptr: as an earlier pass over f left them), then every slice rebuilt
// (unless it is the only one and still in place) and handed to launch(j0, n_slice).
template <typename Launch>
int filter_tested_slices(mdb_ctx *ctx, FilterPass &f, const uint32_t *per_point, unsigned long long *position,
                         unsigned long long *block_sums, Launch launch) {
    if (per_point && filter_gather_tested(ctx, f, per_point, position, block_sums)) return 1;
    for (const auto &range : f.slices) {
        if (!f.kept && filter_rebuild_slice(ctx, f, range.first, range.second)) return 1;
        if (range.second > range.first) launch(range.first, range.second - range.first);
    }
    f.kept = f.slices.size() == 1;
    return 0;
}
// What a count leaves for its write: counts[i] (the rows of segment i of `in`) scanned into offsets (n + 1), and read
// back (one synchronisation) their total and, through by_type (three words in HBM), the rows of every model type:
// rows_created and rows_created_by_model_type of *metrics.
int filter_count_done(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *counts, unsigned long long *offsets,
                      unsigned long long *block_sums, unsigned long long *by_type, const char *scan_name, uint64_t *total,
                      mdb_grid_metrics *metrics);

} // namespace mdb
