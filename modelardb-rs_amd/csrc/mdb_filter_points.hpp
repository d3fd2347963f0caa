// mdb_filter_points.hpp - what the filtered grid (mdb_filter.hip) and the row masks (mdb_mask.hip) share: the three
// classes a time-clipped segment falls into under a value predicate (classify_segment), and the segments whose
// points have to be looked at one by one, gathered into a batch of their own and rebuilt by the range grid in
// bounded slices (FilterPass, filter_gather_tested, filter_rebuild_slice).
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
// by_type[k] (three words in HBM) = the sum of counts[i] over the segments of model type k.
int filter_rows_by_type(mdb_ctx *ctx, const int8_t *types, const uint32_t *counts, uint64_t n,
                        unsigned long long *by_type);

} // namespace mdb
