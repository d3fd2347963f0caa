// mdb_derived.hip - derived fields of two fields (mdb_derived_values*, mdb_derived_buckets*): z = f(x, y) as a column
// and, per date_bin bucket and group, one mdb_derived_cell (count, mean, m2, min, max) of z.
//
// What the reference answers with GridExec per field -> SortedJoinExec -> GeneratedAsExec -> AggregateExec
// (query/generated_as_exec.rs; rows zipped by position, query/sorted_join_exec.rs:278-310). A derived field needs every
// row of both fields whatever the model type - there is no closed form to protect - so this operator decodes no value
// stream of its own: both fields are rebuilt values-only by the range grid into two scratch columns (4 + 4 B per row, in
// HBM only) and the reduction runs over ROWS, not over segments:
//
//   rows and columns       comoments_rows (mdb_comoments.hip): the rows of x and y under [t_lo, t_hi] compared, x's first
//                          rows, the y column; the x column is the range grid of x, values only.
//   k_derived_values       (mdb_derived_values*) z = f(x, y) elementwise, in place where the caller's `values` is
//                          16-byte aligned (the grid of x writes there), 16-byte stores on the aligned body of the output
//                          and a scalar head and tail.
//   k_agg_bucket_span      (shared) the buckets each x segment reaches, its group id checked; a scan makes pair offsets.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS pairs:
//   k_derived_intervals    1 lane / x segment with pairs in the slice: per pair its key and the interval of rows it
//                          holds. Regular timestamps, every model type: O(1) (regular_index_interval and the segment's
//                          first row). Irregular: the timestamps decoded once per segment. A malformed stream whose
//                          timestamps are not sorted has no intervals: its pairs are marked and go point by point.
//                          An interval of at most MDB_DERIVED_SHORT_ROWS rows (and a marked pair) is ONE entry; a longer
//                          one is cut at the multiples of MDB_DERIVED_CHUNK_ROWS in absolute row numbers, one entry per
//                          chunk. A scan over the packed counts gives every pair its first entry and first chunk.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS entries, in row order:
//   k_derived_lanes        1 lane / pair: a short interval reduced by its lane - neighbouring lanes read neighbouring
//                          stretches of the two columns; a marked pair tested timestamp by timestamp.
//   k_derived_waves        1 wave / chunk: 16-byte loads of both columns, f(x, y) formed in registers, every lane a run
//                          of its own, then a reduction of fixed shape (lane l takes lane l + 32, 16, .. 1) under the
//                          merge rule.
//   k_agg_bucket_check, k_derived_tree, k_derived_fold: BucketFold<DerivedFoldOps> (mdb_bucket_fold.hpp), the cells
//                          staged and committed by BucketCells. No two lanes write one cell, no atomics on cells, the
//                          order of every merge fixed by the input, the request and the slice size.
//
// Scratch: 8 B per row (the two columns), 40 B per pair (interval, key, count, offset), 40 B per entry of a slice, 4 B per
// chunk.
#include "mdb_derived.hpp"
#include "mdb_comoments.hpp"
#include "mdb_scan.hpp"

#include <algorithm>
#include <string>

namespace mdb {

// (MDB_DERIVED_SWEEP_SHORT / _CHUNK: other values for the builds of the sweep in MEASUREMENTS.md 37, each on its own;
// the library that ships is built without them and has the constants of mdb.h, which the bindings mirror)
#if defined(MDB_DERIVED_SWEEP_SHORT)
constexpr uint32_t DERIVED_SHORT = MDB_DERIVED_SWEEP_SHORT;
#else
constexpr uint32_t DERIVED_SHORT = MDB_DERIVED_SHORT_ROWS;
#endif
#if defined(MDB_DERIVED_SWEEP_CHUNK)
constexpr uint32_t DERIVED_CHUNK = MDB_DERIVED_SWEEP_CHUNK;
#else
constexpr uint32_t DERIVED_CHUNK = MDB_DERIVED_CHUNK_ROWS;
#endif
constexpr uint32_t DERIVED_UNSORTED = 0xffffffffu; // DerivedInterval::n of a pair that goes point by point
static_assert(DERIVED_CHUNK % (4 * MDB_WAVE) == 0, "a full chunk is a whole number of 16-byte loads per lane");
static_assert(DERIVED_SHORT >= 1 && DERIVED_SHORT < DERIVED_UNSORTED, "the threshold");

__device__ __forceinline__ mdb_derived_cell derived_empty() { return mdb_derived_cell{0, 0.0, 0.0, 0.0f, 0.0f}; }

struct DerivedFoldOps : FoldOps<mdb_derived_cell> {
    static constexpr const char *tree_name = "k_derived_tree", *fold_name = "k_derived_fold";
    __device__ __forceinline__ static mdb_derived_cell empty() { return derived_empty(); }
    __device__ __forceinline__ static void merge(mdb_derived_cell &into, const mdb_derived_cell &from) { derived_merge(into, from); }
    __device__ __forceinline__ static bool is_empty(const mdb_derived_cell &acc) { return acc.count == 0; }
    __device__ __forceinline__ void apply(mdb_derived_cell &cell, const mdb_derived_cell &acc) const { derived_merge(cell, acc); }
};

// The rows [row, row + n) of the two columns a pair holds; n == DERIVED_UNSORTED: no interval (the pair of `segment` is
// tested timestamp by timestamp). Every interval lies inside the columns: k_derived_intervals has checked it.
struct DerivedInterval {
    unsigned long long row;
    uint32_t n;
    uint32_t segment;
};

// The two columns: one f32 per row of the range grids of x and y. Rows are read without a test where an interval has
// been checked against n_rows, and through at() otherwise.
struct DerivedColumns {
    const float *x, *y;
    uint64_t n_rows;
    __device__ __forceinline__ bool at(uint64_t row, float *x_value, float *y_value, uint32_t *error) const {
        if (row < n_rows) {
            *x_value = x[row];
            *y_value = y[row];
            return true;
        }
        *error |= ERR_COMOMENTS_ROW;
        return false;
    }
};

// entries (low word) and chunks (high word) of an interval of n rows at `row`, packed for one scan
__device__ __forceinline__ unsigned long long derived_counts(unsigned long long row, uint32_t n) {
    if (n == DERIVED_UNSORTED || n <= DERIVED_SHORT) return 1ull;
    const unsigned long long chunks = (row + n - 1) / DERIVED_CHUNK - row / DERIVED_CHUNK + 1;
    return chunks << 32 | chunks;
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_derived_intervals(
    DevSegments s, const uint32_t *__restrict__ groups, BucketRequest r, const unsigned long long *__restrict__ offsets,
    uint64_t p0, uint64_t p1, DerivedInterval *__restrict__ intervals, unsigned long long *__restrict__ pair_keys,
    unsigned long long *__restrict__ counts, unsigned int *__restrict__ error_out,
    const unsigned long long *__restrict__ first_row, uint64_t n_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= s.n) return;
    const uint64_t off = offsets[i], stop = offsets[i + 1];
    const uint64_t j0 = off > p0 ? off : p0, j1 = stop < p1 ? stop : p1;
    if (j0 >= j1) return;
    uint64_t b_first = 0;
    (void)bucket_span(s.start_time[i], s.end_time[i], r, &b_first);
    const uint64_t key_row = (uint64_t)(groups ? groups[i] : 0u) * r.n_buckets;
    for (uint64_t j = j0; j < j1; j++) {
        pair_keys[j - p0] = key_row + b_first + (j - off);
        intervals[j - p0] = DerivedInterval{0, 0, (uint32_t)i};
    }
    const SegInfo info = analyse_segment(s, i);
    const SegDesc &d = info.desc;
    uint32_t error = info.error;
    const uint64_t segment_row = first_row[i];
    if (!error && (d.flags & FLAG_REGULAR)) {
        uint32_t k_first = 0, k_last = 0; // the segment's points inside [t_lo, t_hi]: point k_first is its row 0
        (void)regular_index_interval(d.start, d.delta, d.n_total, r.t_lo, r.t_hi, &k_first, &k_last);
        for (uint64_t j = j0; j < j1; j++) {
            int64_t lo, hi;
            bucket_bounds(r, b_first + (j - off), &lo, &hi);
            uint32_t k_lo = 0, k_hi = 0;
            if (regular_index_interval(d.start, d.delta, d.n_total, lo, hi, &k_lo, &k_hi)) {
                intervals[j - p0].row = segment_row - k_first + k_lo;
                intervals[j - p0].n = k_hi - k_lo + 1;
            }
        }
    } else if (!error) {
        // Irregular timestamps, decoded once: pass 1 of comoments_stream_partials.
        const uint4 vt = s.timestamps.views[i];
        uint64_t slot = ~0ull;
        uint32_t k_lo = 0, k_hi = 0, k_first = 0;
        int64_t previous = INT64_MIN;
        bool sorted = true, any_in_range = false;
        auto close = [&]() {
            intervals[slot - p0].row = segment_row - k_first + k_lo;
            intervals[slot - p0].n = k_hi - k_lo + 1;
        };
        decode_irregular_timestamps(view_data(s.timestamps, i, vt), vt.x, d.start, s.end_time[i], 0xffffffffu, &error,
                                    [&](uint32_t k, int64_t t) {
                                        if (t < previous) sorted = false;
                                        previous = t;
                                        if (!sorted || t < r.t_lo || t > r.t_hi) return;
                                        if (!any_in_range) {
                                            any_in_range = true;
                                            k_first = k;
                                        }
                                        if (t < r.origin) return;
                                        const uint64_t b = ((uint64_t)t - (uint64_t)r.origin) / (uint64_t)r.width;
                                        if (b < b_first || b >= r.n_buckets) return;
                                        const uint64_t j = off + (b - b_first);
                                        if (j < j0 || j >= j1) return;
                                        if (j != slot) {
                                            if (slot != ~0ull) close();
                                            slot = j;
                                            k_lo = k;
                                        }
                                        k_hi = k;
                                    });
        if (sorted && slot != ~0ull) close();
        if (!sorted)
            for (uint64_t j = j0; j < j1; j++) intervals[j - p0] = DerivedInterval{0, DERIVED_UNSORTED, (uint32_t)i};
    }
    for (uint64_t j = j0; j < j1; j++) {
        DerivedInterval interval = intervals[j - p0];
        if (error) interval = DerivedInterval{0, 0, (uint32_t)i};
        if (interval.n != DERIVED_UNSORTED && interval.n > 0 &&
            (interval.row >= n_rows || interval.n > n_rows - interval.row)) {
            error |= ERR_COMOMENTS_ROW; // (never with two batches that line up: the call fails, nothing is read)
            interval = DerivedInterval{0, 0, (uint32_t)i};
        }
        intervals[j - p0] = interval;
        counts[j - p0] = derived_counts(interval.row, interval.n);
    }
    if (error) atomicOr(error_out, error);
}

// One pair [lo, hi] of a segment with irregular timestamps that are not sorted (a malformed stream): the points the
// range aggregate counts for the same bounds at the rows segment_range (mdb_agg_dev.hpp) gives them under
// [t_lo, t_hi], as comoments_unsorted_pair. A model without residuals: every point is tested with its own timestamp,
// its row the running count of the points inside [t_lo, t_hi]. Values in a bit stream: the indices between the first
// and the last timestamp inside [lo, hi], point k at row k - the first index inside [t_lo, t_hi].
__device__ __forceinline__ mdb_derived_cell derived_unsorted_pair(const DevSegments &s, uint64_t i, const BucketRequest &r,
                                                                  int64_t lo, int64_t hi, uint64_t first_row,
                                                                  const DerivedColumns &columns,
                                                                  const mdb_derived_expr &expr, uint32_t *error) {
    const SegInfo info = analyse_segment(s, i);
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    const int64_t end = s.end_time[i];
    const uint4 vt = s.timestamps.views[i];
    const uint8_t *ts_bytes = view_data(s.timestamps, i, vt);
    DerivedRun run = derived_run_empty();
    float x = 0.0f, y = 0.0f;
    if (end < lo || d.start > hi) return derived_finish(run);
    if (type != MDB_MACAQUE_V_ID && d.n_total == d.n_model) {
        uint64_t row = first_row;
        decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t, int64_t t) {
            if (t < r.t_lo || t > r.t_hi) return;
            if (t >= lo && t <= hi && columns.at(row, &x, &y, error)) derived_point(run, derived_eval(expr, x, y));
            row += 1;
        });
        return derived_finish(run);
    }
    uint32_t k_lo = 0xffffffffu, k_hi = 0, k_first = 0xffffffffu;
    decode_irregular_timestamps(ts_bytes, vt.x, d.start, end, 0xffffffffu, error, [&](uint32_t k, int64_t t) {
        if (t >= r.t_lo && t <= r.t_hi && k < k_first) k_first = k;
        if (t >= lo && t <= hi) {
            if (k < k_lo) k_lo = k;
            if (k > k_hi) k_hi = k;
        }
    });
    if (k_lo == 0xffffffffu) return derived_finish(run); // (else k_first is set as well: [lo, hi] lies inside [t_lo, t_hi])
    for (uint32_t k = k_lo;; k++) {
        if (columns.at(first_row - k_first + k, &x, &y, error)) derived_point(run, derived_eval(expr, x, y));
        if (k == k_hi) break;
    }
    return derived_finish(run);
}

// Pairs [0, m) of the slice; entries [e0, e1) of it are written (entry e at e - e0). One lane per pair: the pairs of one
// entry - a short interval, or a marked pair.
__global__ __launch_bounds__(BUCKET_THREADS) void k_derived_lanes(
    DevSegments s, BucketRequest r, const DerivedInterval *__restrict__ intervals,
    const unsigned long long *__restrict__ pair_keys, const unsigned long long *__restrict__ entry_offsets, uint64_t m,
    uint64_t e0, uint64_t e1, DerivedColumns columns, mdb_derived_expr expr,
    const unsigned long long *__restrict__ first_row, uint32_t *__restrict__ chunk_pair,
    unsigned long long *__restrict__ keys, mdb_derived_cell *__restrict__ out, unsigned int *__restrict__ error_out) {
    const uint64_t j = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (j >= m) return;
    const DerivedInterval interval = intervals[j];
    if (interval.n != DERIVED_UNSORTED && interval.n > DERIVED_SHORT) {
        // (k_derived_waves': its chunks are told their pair, once per slice of pairs)
        const uint64_t q0 = entry_offsets[j] >> 32, q1 = entry_offsets[j + 1] >> 32;
        for (uint64_t q = q0; e0 == 0 && q < q1; q++) chunk_pair[q] = (uint32_t)j;
        return;
    }
    const uint64_t e = entry_offsets[j] & 0xffffffffull;
    if (e < e0 || e >= e1) return;
    const unsigned long long key = pair_keys[j];
    mdb_derived_cell cell;
    if (interval.n == DERIVED_UNSORTED) {
        uint32_t error = 0;
        int64_t lo, hi;
        bucket_bounds(r, key % r.n_buckets, &lo, &hi);
        cell = derived_unsorted_pair(s, interval.segment, r, lo, hi, first_row[interval.segment], columns, expr, &error);
        if (error) atomicOr(error_out, error);
    } else {
        DerivedRun run = derived_run_empty();
        const float *x = columns.x + interval.row, *y = columns.y + interval.row;
        for (uint32_t k = 0; k < interval.n; k++) derived_point(run, derived_eval(expr, x[k], y[k]));
        cell = derived_finish(run);
    }
    keys[e - e0] = key;
    out[e - e0] = cell;
}

__device__ __forceinline__ mdb_derived_cell derived_shfl_down(const mdb_derived_cell &cell, int delta) {
    mdb_derived_cell other;
    other.count = __shfl_down((long long)cell.count, delta);
    other.mean = __shfl_down(cell.mean, delta);
    other.m2 = __shfl_down(cell.m2, delta);
    other.min = __shfl_down(cell.min, delta);
    other.max = __shfl_down(cell.max, delta);
    return other;
}

// One wave per chunk q of the slice's long intervals, n_chunks of them: chunk_pair[q] is its pair (the scanned counts'
// high words give the pair's first chunk), the chunk's rows are read with 16-byte loads - groups of four rows at
// multiples of four, lane l taking groups l, l + 64, ...; a group the interval covers in part is read row by row - and
// the lanes' cells are merged in a fixed shape. Lane 0 writes the entry.
__global__ __launch_bounds__(BUCKET_THREADS) void k_derived_waves(
    const DerivedInterval *__restrict__ intervals, const unsigned long long *__restrict__ pair_keys,
    const unsigned long long *__restrict__ entry_offsets, const uint32_t *__restrict__ chunk_pair, uint64_t m,
    uint64_t n_chunks, uint64_t e0, uint64_t e1, DerivedColumns columns, mdb_derived_expr expr,
    unsigned long long *__restrict__ keys, mdb_derived_cell *__restrict__ out) {
    const int lane = threadIdx.x % MDB_WAVE;
    const uint64_t q = (uint64_t)blockIdx.x * (BUCKET_THREADS / MDB_WAVE) + threadIdx.x / MDB_WAVE;
    if (q >= n_chunks) return;
    const uint64_t a = chunk_pair[q]; // (k_derived_lanes has written it: no bisection in the scanned counts, 18 dependent loads)
    if (a >= m) return;
    const unsigned long long packed = entry_offsets[a];
    const uint64_t chunk = q - (packed >> 32);
    const uint64_t e = (packed & 0xffffffffull) + chunk;
    if (e < e0 || e >= e1) return;
    const DerivedInterval interval = intervals[a];
    const uint64_t end = interval.row + interval.n;
    const uint64_t cut = (interval.row / DERIVED_CHUNK + chunk) * DERIVED_CHUNK;
    const uint64_t r0 = cut > interval.row ? cut : interval.row;
    const uint64_t r1 = cut + DERIVED_CHUNK < end ? cut + DERIVED_CHUNK : end;
    DerivedRun run = derived_run_empty();
    auto four = [&](const float4 &x, const float4 &y) {
        derived_point(run, derived_eval(expr, x.x, y.x));
        derived_point(run, derived_eval(expr, x.y, y.y));
        derived_point(run, derived_eval(expr, x.z, y.z));
        derived_point(run, derived_eval(expr, x.w, y.w));
    };
    if (r0 == cut && r1 == cut + DERIVED_CHUNK) {
        // a whole chunk: every load is issued before the first value is used
        constexpr int ROUNDS = DERIVED_CHUNK / (4 * MDB_WAVE);
        const float4 *x4 = reinterpret_cast<const float4 *>(columns.x + cut) + lane;
        const float4 *y4 = reinterpret_cast<const float4 *>(columns.y + cut) + lane;
        float4 x[ROUNDS], y[ROUNDS];
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            x[k] = x4[k * MDB_WAVE];
            y[k] = y4[k * MDB_WAVE];
        }
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) four(x[k], y[k]);
    } else {
        for (uint64_t g = (r0 & ~3ull) + 4ull * lane; g < r1; g += 4ull * MDB_WAVE) {
            if (g >= r0 && g + 4 <= r1) {
                four(*reinterpret_cast<const float4 *>(columns.x + g), *reinterpret_cast<const float4 *>(columns.y + g));
            } else {
                for (uint64_t row = g > r0 ? g : r0; row < g + 4 && row < r1; row++)
                    derived_point(run, derived_eval(expr, columns.x[row], columns.y[row]));
            }
        }
    }
    mdb_derived_cell cell = derived_finish(run);
#pragma unroll
    for (int delta = MDB_WAVE / 2; delta >= 1; delta /= 2) {
        const mdb_derived_cell other = derived_shfl_down(cell, delta);
        if (lane < delta) derived_merge(cell, other);
    }
    if (lane == 0) {
        keys[e - e0] = pair_keys[a];
        out[e - e0] = cell;
    }
}

// out[k] = f(x[k], y[k]), k < n; x may be out (in place). The body is the 16-byte aligned part of `out`; x and y are read
// there with loads that need 4-byte alignment only (they are 16-byte aligned whenever out is: the columns are).
constexpr int VALUES_THREADS = 256;
__global__ __launch_bounds__(VALUES_THREADS) void k_derived_values(const float *x, const float *__restrict__ y, float *out,
                                                                   uint64_t n, mdb_derived_expr expr) {
    const uint64_t misaligned = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u;
    const uint64_t head = misaligned / 4 < n ? misaligned / 4 : n;
    const uint64_t groups = (n - head) / 4;
    const uint64_t t = (uint64_t)blockIdx.x * VALUES_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * VALUES_THREADS;
    for (uint64_t g = t; g < groups; g += stride) {
        const uint64_t k = head + 4 * g;
        float4 a, b, z;
        __builtin_memcpy(&a, x + k, 16);
        __builtin_memcpy(&b, y + k, 16);
        z.x = derived_eval(expr, a.x, b.x);
        z.y = derived_eval(expr, a.y, b.y);
        z.z = derived_eval(expr, a.z, b.z);
        z.w = derived_eval(expr, a.w, b.w);
        *reinterpret_cast<float4 *>(out + k) = z;
    }
    // (the head and the tail: at most 3 + 3 values, rows no group has touched)
    const uint64_t tail = head + 4 * groups;
    if (t < head) out[t] = derived_eval(expr, x[t], y[t]);
    if (t < n - tail) out[tail + t] = derived_eval(expr, x[tail + t], y[tail + t]);
}

static int capacity_too_small(uint64_t n_rows, uint64_t capacity) {
    return fail("The derived column has " + std::to_string(n_rows) + " rows under the time range but the capacity is " +
                std::to_string(capacity) + ".");
}

// The two columns under [t_lo, t_hi] (comoments_rows: row counts compared, x's first rows, the y column) - `x_out`:
// where the x column goes (16-byte aligned; with its timestamps when x_ts is given), nullptr: into scratch
// (SCRATCH_DERIVED_XCOL). `capacity`: of the caller's outputs, checked before anything is written.
static int derived_columns(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, int64_t t_lo, int64_t t_hi,
                           const unsigned long long **first_row, DerivedColumns *columns, const uint64_t *capacity,
                           int64_t *x_ts, float *x_out) {
    YColumn y_column{nullptr, 0};
    if (comoments_rows(ctx, x, y, t_lo, t_hi, first_row, &y_column)) return 1;
    const uint64_t n_rows = y_column.n_rows;
    if (capacity && *capacity < n_rows) return capacity_too_small(n_rows, *capacity);
    const uint64_t bytes = n_rows * 8;
    if (ctx->scratch_limit && bytes > ctx->scratch_limit)
        return fail("The two columns of " + std::to_string(n_rows) + " rows need " + std::to_string(bytes) +
                    " bytes of scratch but the context's limit is " + std::to_string(ctx->scratch_limit) +
                    ": cut the batch by series.");
    *columns = DerivedColumns{y_column.values, y_column.values, n_rows};
    if (n_rows == 0) return 0;
    if (y == x && !x_out && !x_ts) return 0; // (one field against itself: one column read twice)
    float *values = x_out;
    if (!values) {
        void *p = nullptr;
        if (scratch_reserve(ctx, SCRATCH_DERIVED_XCOL, n_rows * 4, &p)) return 1;
        values = static_cast<float *>(p);
    }
    uint64_t written = 0;
    if (grid_batch_dev_locked(ctx, x, TimeRange{t_lo, t_hi, 1}, x_ts, values, nullptr, n_rows, &written, nullptr)) return 1;
    if (written != n_rows) return fail("The range grid of the x field changed its row count between two passes.");
    columns->x = values;
    return 0;
}

// mdb_derived_values_dev on device batches and device outputs (the context locked, the device selected).
static int derived_values_run(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const mdb_derived_expr &expr,
                              int64_t t_lo, int64_t t_hi, int64_t *timestamps, float *values, uint64_t capacity,
                              uint64_t *rows_out) {
    const unsigned long long *first_row = nullptr;
    DerivedColumns columns{nullptr, nullptr, 0};
    const bool in_place = (reinterpret_cast<uintptr_t>(values) & 15u) == 0;
    if (derived_columns(ctx, x, y, t_lo, t_hi, &first_row, &columns, &capacity, timestamps, in_place ? values : nullptr)) return 1;
    const uint64_t n = columns.n_rows;
    if (n > 0) {
        if (!values) return fail("values must not be NULL.");
        const uint64_t blocks = std::min<uint64_t>((n / 4 + VALUES_THREADS) / VALUES_THREADS, 1u << 16);
        {
            LaunchTimer timer(ctx, "k_derived_values");
            hipLaunchKernelGGL(k_derived_values, dim3((uint32_t)blocks), dim3(VALUES_THREADS), 0, ctx->stream, columns.x, columns.y,
                               values, n, expr);
        }
        MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        MDB_HIP_CHECK(hipGetLastError());
    }
    *rows_out = n;
    return 0;
}

int derived_values_host_run(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y, const mdb_derived_expr *expr,
                            int64_t t_lo, int64_t t_hi, int64_t *timestamps, float *values, uint64_t capacity,
                            uint64_t *rows_out) {
    UploadedSegments lists(ctx);
    if (lists.upload_pair(&x, 1, &y, 1, nullptr)) return 1;
    uint64_t n = 0;
    if (grid_range_plan(ctx, lists.segments(), t_lo, t_hi, &n, nullptr, nullptr)) return 1;
    if (capacity < n) return capacity_too_small(n, capacity);
    void *p = nullptr;
    const uint64_t value_bytes = align_up(n * 4, 256);
    if (scratch_reserve(ctx, SCRATCH_DERIVED_OUT, value_bytes + (timestamps ? n * 8 : 0) + 256, &p)) return 1;
    float *dev_values = static_cast<float *>(p);
    int64_t *dev_ts = timestamps ? reinterpret_cast<int64_t *>(static_cast<uint8_t *>(p) + value_bytes) : nullptr;
    uint64_t rows = 0;
    if (derived_values_run(ctx, lists.segments(), lists.y_segments(), *expr, t_lo, t_hi, dev_ts, dev_values, capacity, &rows))
        return 1;
    if (rows > 0) {
        if (!values) return fail("values must not be NULL.");
        MDB_HIP_CHECK(hipMemcpyAsync(values, dev_values, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (timestamps) MDB_HIP_CHECK(hipMemcpyAsync(timestamps, dev_ts, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
        MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    *rows_out = rows;
    return 0;
}

// The buckets of the device batches x and y (groups: a device array or nullptr) merged into a device array of n_cells
// cells. `host_cells` (host forms): the caller's array, which is uploaded, merged into and downloaded instead; either
// way nothing of the caller's is written unless the whole call succeeds.
static int derived_run(mdb_ctx *ctx, const mdb_segments *in, const mdb_segments *y_in, const uint32_t *groups,
                       const mdb_bucket_request *request, const mdb_derived_expr &expr, uint64_t n_cells,
                       mdb_derived_cell *dev_cells, mdb_derived_cell *host_cells) {
    const uint64_t n = in->n;
    if (n == 0 || request->n_buckets == 0 || request->t_lo > request->t_hi) return 0;
    const BucketRequest r = {request->origin, request->width, request->n_buckets, request->t_lo, request->t_hi,
                             request->n_groups, request->which_mask};
    if (n > UINT64_MAX / request->n_buckets)
        return fail("Too many (segment, bucket) pairs for one call: split the batch.");
    const unsigned long long *first_row = nullptr;
    DerivedColumns columns{nullptr, nullptr, 0};
    if (derived_columns(ctx, in, y_in, r.t_lo, r.t_hi, &first_row, &columns, nullptr, nullptr, nullptr)) return 1;
    const DevSegments s = to_dev(in);
    const unsigned long long *offsets = nullptr;
    unsigned int *words = nullptr;
    unsigned long long total = 0;
    if (bucket_span_pairs(ctx, in, s, groups, r, &offsets, &words, &total)) return 1;
    if (total == 0) return 0;

    const uint64_t slice = slice_pairs_setting();
    const uint64_t pair_cap = std::min<uint64_t>(slice, total);
    // (an interval of n rows makes at most n / CHUNK + 2 entries)
    const uint64_t most_entries = 2 * total + columns.n_rows / DERIVED_CHUNK;
    if (2 * pair_cap + columns.n_rows / DERIVED_CHUNK > 0xffffffffull)
        return fail("Too many rows for the pairs of one slice: lower MDB_AGG_BUCKET_SLICE_PAIRS or cut the batch by series.");
    const uint64_t entry_cap = std::min<uint64_t>(slice, most_entries);
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_DERIVED_PAIRS,
                        align_up(pair_cap * sizeof(DerivedInterval), 256) + 3 * align_up((pair_cap + 1) * 8, 256) +
                            align_up(scan_block_sums_bytes(pair_cap), 256),
                        &p))
        return 1;
    Carver scratch(p);
    DerivedInterval *intervals = scratch.take<DerivedInterval>(pair_cap);
    unsigned long long *pair_keys = scratch.take<unsigned long long>(pair_cap + 1);
    unsigned long long *counts = scratch.take<unsigned long long>(pair_cap + 1);
    unsigned long long *entry_offsets = scratch.take<unsigned long long>(pair_cap + 1);
    unsigned long long *block_sums = scratch.take<unsigned long long>(scan_block_sums_bytes(pair_cap) / 8);

    BucketCells<mdb_derived_cell> cells;
    if (cells.stage(ctx, n_cells, dev_cells, host_cells, total <= slice && most_entries <= slice ? 1 : 2)) return 1;
    BucketFold<DerivedFoldOps> fold;
    if (fold.reserve(ctx, entry_cap, n_cells)) return 1;
    mdb_derived_cell *partials = fold.partials();
    unsigned long long *keys = fold.keys();

    for (uint64_t p0 = 0; p0 < total; p0 += slice) {
        const uint64_t p1 = std::min<uint64_t>(p0 + slice, total), m = p1 - p0;
        MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
        {
            LaunchTimer timer(ctx, "k_derived_intervals");
            hipLaunchKernelGGL(k_derived_intervals, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, r,
                               offsets, p0, p1, intervals, pair_keys, counts, words, first_row, columns.n_rows);
        }
        if (device_exclusive_scan(ctx, ItemsOf<unsigned long long>{counts}, m, entry_offsets, block_sums, "k_derived_scan"))
            return 1;
        unsigned long long packed = 0;
        MDB_HIP_CHECK(hipMemcpyAsync(&packed, entry_offsets + m, 8, hipMemcpyDeviceToHost, ctx->stream));
        MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const uint64_t entries = packed & 0xffffffffull, chunks = packed >> 32;
        if (std::min<uint64_t>(entries, slice) > entry_cap || chunks > entries)
            return fail("(internal) The row intervals of a slice overlap: more entries than its rows can make.");
        uint32_t *chunk_pair = nullptr; // per chunk of the slice's long intervals its pair
        if (chunks > 0) {
            if (scratch_reserve(ctx, SCRATCH_DERIVED_CHUNKS, chunks * 4, &p)) return 1;
            chunk_pair = static_cast<uint32_t *>(p);
        }
        // Every slice of entries launches k_derived_lanes over all m pairs and k_derived_waves over all chunks of the
        // slice of pairs; a lane or wave whose entry lies outside [e0, e1) reads its pair's offset and returns. With the
        // default slice size there is one slice of entries; a small MDB_AGG_BUCKET_SLICE_PAIRS (the tests') costs
        // slices x entries of such returns.
        for (uint64_t e0 = 0; e0 < entries; e0 += slice) {
            const uint64_t e1 = std::min<uint64_t>(e0 + slice, entries);
            if (e0 > 0) MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
            {
                LaunchTimer timer(ctx, "k_derived_lanes");
                hipLaunchKernelGGL(k_derived_lanes, dim3(blocks_for(m)), dim3(BUCKET_THREADS), 0, ctx->stream, s, r, intervals,
                                   pair_keys, entry_offsets, m, e0, e1, columns, expr, first_row, chunk_pair, keys, partials, words);
            }
            if (chunks > 0) {
                const uint64_t per_block = BUCKET_THREADS / MDB_WAVE;
                LaunchTimer timer(ctx, "k_derived_waves");
                hipLaunchKernelGGL(k_derived_waves, dim3((uint32_t)((chunks + per_block - 1) / per_block)), dim3(BUCKET_THREADS),
                                   0, ctx->stream, intervals, pair_keys, entry_offsets, chunk_pair, m, chunks, e0, e1, columns, expr,
                                   keys, partials);
            }
            unsigned int error = 0;
            bool unsorted = false;
            if (bucket_slice_check(ctx, keys, e1 - e0, words, &error, &unsorted)) return 1;
            if (error & ERR_COMOMENTS_ROW)
                return fail("(internal) A row of the x field lies beyond the columns: the row plan and the range grid "
                            "disagree.");
            if (error) return fail(describe_error(error));
            if (fold.fold_slice(ctx, e1 - e0, unsorted, cells.cells())) return 1;
        }
    }
    return cells.commit();
}

int derived_list_run(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys,
                     uint32_t n_y, const uint32_t *const *group_of_segment_x, const mdb_bucket_request *request,
                     const mdb_derived_expr *expr, uint64_t n_cells, mdb_derived_cell *inout) {
    // (uploads the library holds, as mdb_comoments_buckets_list)
    UploadedSegments lists(ctx);
    if (lists.upload_pair(xs, n_x, ys, n_y, group_of_segment_x)) return 1;
    return derived_run(ctx, lists.segments(), lists.y_segments(), lists.groups(), request, *expr, n_cells, nullptr, inout);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_derived_buckets_dev(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y,
                                       const uint32_t *group_of_segment_x, const mdb_bucket_request *request,
                                       const mdb_derived_expr *expr, mdb_derived_cell *inout) {
    if (!ctx || !x || !y || !request || !expr || !inout)
        return fail("ctx, x, y, request, expr and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (derived_request_check(request, &n_cells) || derived_expr_check(expr)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return derived_run(ctx, x, y, group_of_segment_x, request, *expr, n_cells, inout, nullptr);
}

extern "C" int mdb_derived_values_dev(mdb_ctx *ctx, const mdb_segments *x, const mdb_segments *y,
                                      const mdb_derived_expr *expr, int64_t t_lo, int64_t t_hi, int64_t *timestamps,
                                      float *values, uint64_t capacity, uint64_t *rows_out) {
    if (!ctx || !x || !y || !expr || !rows_out) return fail("ctx, x, y, expr and rows_out must not be NULL.");
    if (derived_expr_check(expr)) return 1;
    if (reinterpret_cast<uintptr_t>(values) & 3u) return fail("values must be 4-byte aligned.");
    if (x->n == 0 || t_lo > t_hi) {
        *rows_out = 0;
        return 0;
    }
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return derived_values_run(ctx, x, y, *expr, t_lo, t_hi, timestamps, values, capacity, rows_out);
}
