// mdb_hist_dev.hpp - what one lane of the histogram kernels carries from point to point, shared by k_hist (mdb_hist.hip:
// cells per group) and k_hist_buckets (mdb_hist_buckets.hip: cells per group and date_bin bucket, and the windowed cells
// of the per-bucket quantiles): the lane of a cell rule, and the selector of segment_range that counts into it.
//
// A lane type gives: cell_of(key), monotone in the key; add(key, n); flush(); and the members lo / hi (the closed key
// interval of the current cell), cell and run, which HistCellsOf::model reads and moves for a Swing run.
#pragma once

#include "mdb_agg_dev.hpp"
#include "mdb_filter.hpp"
#include "mdb_segment_dev.hpp"
#include "mdb_select.hpp"

namespace mdb {

constexpr int HIST_THREADS = 256;
constexpr uint32_t ERR_HIST_GROUP = 1u << 31; // a group id >= n_groups

// The workgroups of a histogram kernel over n items: grid-stride beyond 8 workgroups per CU, as the aggregates.
inline uint32_t hist_blocks(uint64_t n) {
    const uint64_t blocks = (n + HIST_THREADS - 1) / HIST_THREADS;
    return (uint32_t)(blocks < 256 * 8 ? blocks : 256 * 8);
}

// The lane of an edge list: the cell of a key is the number of edges at or below it.
struct HistLane {
    const int32_t *edges;      // the edges' keys (LDS)
    uint32_t n_edges;
    unsigned long long *cells; // the row of the segment's group (and bucket)
    int32_t lo, hi;            // the keys of the current cell, closed (lo > hi: no cell yet)
    uint32_t cell;
    unsigned long long run;    // points of the current cell not added yet

    // The number of edges at or below `key`.
    __device__ __forceinline__ uint32_t cell_of(int32_t key) const {
        uint32_t a = 0, b = n_edges;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (edges[mid] <= key) a = mid + 1;
            else b = mid;
        }
        return a;
    }
    __device__ __forceinline__ void flush() {
        if (run) atomicAdd(&cells[cell], run);
        run = 0;
    }
    // n points of key `key` (n may be 0: the lane's cell becomes the key's).
    __device__ __forceinline__ void add(int32_t key, unsigned long long n) {
        if (key < lo || key > hi) {
            flush();
            cell = cell_of(key);
            lo = cell == 0 ? INT32_MIN : edges[cell - 1];
            hi = cell == n_edges ? INT32_MAX : edges[cell] - 1; // (edges[cell] > key: no wrap)
        }
        run += n;
    }
};

// The lane of a pass of the radix selection (mdb_select.hpp): a row holds n_ranks windows of SELECT_DIGITS counters. The
// "cell" of a key is its unsigned key above `shift` - the bits every rank has pinned so far and the digit this pass
// counts by - so cells are arithmetic, monotone in the key, and a run of one cell is added to the window of every rank
// whose prefix it carries, under its digit. Pass 0 (shift 24, prefixes == nullptr): no bit is pinned, one window.
struct WindowLane {
    const uint32_t *prefixes;  // of the current row: n_ranks prefixes (the bits above the digit)
    uint32_t n_ranks;
    uint32_t shift;
    unsigned long long *cells; // the row: n_ranks * SELECT_DIGITS counters
    int32_t lo, hi;
    uint32_t cell;
    unsigned long long run;

    __device__ __forceinline__ uint32_t cell_of(int32_t key) const { return select_ukey(key) >> shift; }
    __device__ __forceinline__ void flush() {
        if (run) {
            const uint32_t digit = cell & (SELECT_DIGITS - 1), above = cell >> SELECT_DIGIT_BITS;
            for (uint32_t rank = 0; rank < n_ranks; rank++)
                if (!prefixes || prefixes[rank] == above) atomicAdd(&cells[rank * SELECT_DIGITS + digit], run);
        }
        run = 0;
    }
    __device__ __forceinline__ void add(int32_t key, unsigned long long n) {
        if (key < lo || key > hi) {
            flush();
            cell = cell_of(key);
            const uint32_t first = cell << shift;
            lo = select_key_of_ukey(first);
            hi = select_key_of_ukey(first | ((1u << shift) - 1u));
        }
        run += n;
    }
};

// The selector of segment_range (mdb_filter.hpp) that counts into cells: counts() records the point and selects
// nothing (the walk's RangeAcc stays empty), model() is the closed form over the model points [a, b].
template <typename Lane>
struct HistCellsOf {
    static constexpr bool by_row = false;
    Lane *lane;
    __device__ __forceinline__ bool counts(float v, uint64_t) const {
        lane->add(total_order_key(__float_as_uint(v)), 1);
        return false;
    }
    __device__ __forceinline__ void model(const SegDesc &d, uint32_t type, uint32_t a, uint32_t b, uint64_t,
                                          RangeAcc &) const {
        Lane &l = *lane;
        const uint32_t n = b - a + 1;
        if (type == MDB_PMC_MEAN_ID) {
            l.add(total_order_key(__float_as_uint(d.value)), n);
            return;
        }
        auto key_at = [&](uint32_t k) { return total_order_key(__float_as_uint(swing_value_at(d, k))); };
        auto point_by_point = [&]() {
            for (uint32_t k = a;; k++) {
                l.add(key_at(k), 1);
                if (k == b) break;
            }
        };
        const float va = swing_value_at(d, a), vb = swing_value_at(d, b);
        if (va != va || vb != vb) return point_by_point(); // (as ValueKeys::model: the run is not known to be sorted)
        const int32_t ka = total_order_key(__float_as_uint(va)), kb = total_order_key(__float_as_uint(vb));
        const uint32_t ca = l.cell_of(ka), cb = l.cell_of(kb);
        if (ca == cb) { // (slope 0, or a line that stays inside one cell: the keys between the ends lie between them)
            l.add(ka, n);
            return;
        }
        const uint32_t crossed = ca < cb ? cb - ca : ca - cb;
        const uint32_t steps = 32u - (uint32_t)__clz(n - 1); // ceil(log2(n)), n >= 2 here: the steps of one search
        if ((uint64_t)crossed * steps > n) return point_by_point();
        // The keys are sorted along k (model_run): walk from the first end's cell to the last end's, each crossed edge's
        // first index found by one binary search.
        const bool up = ka < kb;
        uint32_t at = a;
        while (at <= b) {
            l.add(key_at(at), 0);
            if (l.cell == cb) {
                l.run += b + 1 - at;
                break;
            }
            const int32_t lo = l.lo, hi = l.hi;
            const uint32_t next = up ? swing_first_past(d, at + 1, b + 1, [&](int32_t key) { return key > hi; })
                                     : swing_first_past(d, at + 1, b + 1, [&](int32_t key) { return key < lo; });
            l.run += next - at;
            at = next;
        }
    }
};
using HistCells = HistCellsOf<HistLane>;

// Does segment i keep per-bucket index intervals in slots? Irregular timestamps and values in a bit stream, judged by
// the views alone (a superset of what analyse_segment finds: a residual view that holds no point still gets slots).
__device__ __forceinline__ bool hist_bucket_wants_slots(const DevSegments &s, uint64_t i) {
    if (segment_has_regular_timestamps(s, i) || (int32_t)s.timestamps.views[i].x <= 0) return false;
    return s.model_type_id[i] == MDB_MACAQUE_V_ID || (int32_t)s.residuals.views[i].x > 0;
}

struct HistSlotCount { // the functor of the scan
    DevSegments s;
    BucketRequest r;
    __device__ uint64_t operator()(uint64_t i) const {
        if (!hist_bucket_wants_slots(s, i)) return 0;
        uint64_t first = 0;
        return bucket_span(s.start_time[i], s.end_time[i], r, &first);
    }
};

struct HistSlots { // the slots of the segments with irregular timestamps under bit-stream values
    const unsigned long long *offsets = nullptr;
    uint2 *slots = nullptr;
};

// mdb_hist_buckets.hip (mdb_binned.hip too): counters or slots that cannot fit the device are an error, asked only where
// it could matter; k_hist_bucket_slots' scan and the slots themselves (SCRATCH_HIST_BUCKET_OFFSETS / _SLOTS).
int hist_buckets_fits(uint64_t bytes, const char *what);
int hist_buckets_slots(mdb_ctx *ctx, const mdb_segments *in, const DevSegments &s, const BucketRequest &r, HistSlots *out);

// mdb_hist.hip, for the callers of mdb_hist_buckets.hip: k_hist_groups over the n ids of `groups` (sets ERR_HIST_GROUP in
// *error), and k_hist_fold (counts[j] += cells[j] where cells[j] != 0), both enqueued on the context's stream.
void hist_groups_launch(mdb_ctx *ctx, const uint32_t *groups, uint64_t n, uint32_t n_groups, unsigned int *error);
void hist_fold_launch(mdb_ctx *ctx, const unsigned long long *cells, uint64_t n, unsigned long long *counts);

} // namespace mdb
