// mdb_integral.hip - time-weighted averages and integrals per date_bin bucket and group, computed on segments
// (mdb_integral_buckets*): per cell the microseconds on which the series is defined and the integral of the series
// over them, under LINEAR (trapezoid) or STEP (last observation carried forward) interpolation between linked rows.
//
// What the reference can only answer with GridExec -> WindowAggExec(lag) -> AggregateExec over every rebuilt point.
// Here a (segment, bucket) pair is O(1) for PMC-Mean (value x clipped duration) and for Swing (a closed form of the
// line's point sums) on regular timestamps. The one new problem is the interval between a segment's last point and
// its right neighbour's first: it belongs to the left segment, whose extent and pairs reach over it.
//
//   k_integral_span      (in place of k_agg_bucket_span, through bucket_span_pairs) 1 lane / segment: the buckets its
//                        extent [start_time, linked ? start_time of the next : end_time] overlaps, its group id checked.
//   k_integral_heads     1 lane / segment whose left neighbour has pairs and shares its group: the value of its first
//                        point (its time is start_time), 8 B of scratch. A pass of its own: the second
//                        analyse_segment stays out of the hot kernel.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS pairs, slices folded one after the other:
//   k_integral_partials  1 lane / segment with pairs in the slice: one {key, cell} per pair (mdb_integral.hpp).
//   k_agg_bucket_check   (shared) keys non-decreasing? If not, a stable radix sort by key.
//   k_integral_tree, k_integral_fold  k_agg_bucket_tree / k_agg_bucket_fold for a {u64, f64} partial added member by
//                        member: runs of equal keys reduced through the fixed tree of 64-entry tiles and merged into
//                        the cells by the lane of each run's last pair. No two lanes write one cell, no float atomics,
//                        every addition's order fixed by the pair order.
// Every stream is one lane's: the batch's cursor index (k_*_pieces) is not used.
//
// Scratch: 16 B per pair (the cell) and the 8-byte key, written and read back; 8 B per segment of heads.
#include "mdb_integral.hpp"
#include "mdb_scan.hpp"

#include <algorithm>
#include <vector>

namespace mdb {

struct IntegralTree { // level 0 is the slice's pairs (keys, cells, and the sort's pair numbers); 1.. are the tree's
    const unsigned long long *keys[BUCKET_MAX_LEVELS];
    const mdb_integral_cell *values[BUCKET_MAX_LEVELS];
    uint64_t n[BUCKET_MAX_LEVELS];
    const uint32_t *order; // (level 0 in key order: values[0][order[j]]; nullptr: pair order)
    int levels;
};

__global__ __launch_bounds__(BUCKET_THREADS) void k_integral_span(DevSegments s, const uint32_t *__restrict__ groups,
                                                                  IntegralRequest q,
                                                                  unsigned long long *__restrict__ counts,
                                                                  unsigned int *__restrict__ error) {
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= s.n) return;
    uint64_t first = 0;
    uint64_t count = integral_span(s, groups, i, q, &first);
    if (groups && groups[i] >= q.buckets.n_groups) {
        atomicOr(error, ERR_BUCKET_GROUP);
        count = 0;
    }
    counts[i] = count;
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_integral_heads(DevSegments s, const uint32_t *__restrict__ groups,
                                                                   const unsigned long long *__restrict__ offsets,
                                                                   IntegralHead *__restrict__ heads,
                                                                   unsigned int *__restrict__ error_out) {
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i == 0 || i >= s.n) return;
    if (offsets[i] == offsets[i - 1] || !integral_same_group(groups, i - 1, i)) return; // (never read)
    const SegInfo info = analyse_segment(s, i);
    uint32_t error = info.error;
    heads[i] = error ? IntegralHead{0.0f, info.desc.n_total} : integral_head_of(s, i, info, &error);
    if (error) atomicOr(error_out, error);
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_integral_partials(DevSegments s, const uint32_t *__restrict__ groups,
                                                                      IntegralRequest q,
                                                                      const unsigned long long *__restrict__ offsets,
                                                                      uint64_t p0, uint64_t p1,
                                                                      const IntegralHead *__restrict__ heads,
                                                                      mdb_integral_cell *__restrict__ out,
                                                                      unsigned long long *__restrict__ keys,
                                                                      unsigned int *__restrict__ error_out) {
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= s.n) return;
    const uint64_t off = offsets[i], stop = offsets[i + 1];
    const uint64_t j0 = off > p0 ? off : p0, j1 = stop < p1 ? stop : p1;
    if (j0 >= j1) return;
    uint64_t b_first = 0;
    (void)integral_span(s, groups, i, q, &b_first);
    const uint64_t row = (uint64_t)(groups ? groups[i] : 0u) * q.buckets.n_buckets;
    for (uint64_t j = j0; j < j1; j++) keys[j - p0] = row + b_first + (j - off);
    const SegInfo info = analyse_segment(s, i);
    uint32_t error = info.error;
    if (error) {
        for (uint64_t j = j0; j < j1; j++) out[j - p0] = mdb_integral_cell{0, 0.0}; // (the call fails)
    } else {
        const bool neighbour = i + 1 < s.n && integral_same_group(groups, i, i + 1);
        integral_segment_partials(s, i, info, q, off, b_first, j0, j1, p0, out, neighbour, heads, &error);
    }
    if (error) atomicOr(error_out, error);
}

__device__ __forceinline__ mdb_integral_cell integral_value(const IntegralTree &tree, int level, uint64_t t) {
    return tree.values[level][level == 0 && tree.order ? tree.order[t] : t];
}

// Level `level` + 1 from `level`: per tile of BUCKET_TILE entries its last key and the sum of the run ending it.
__global__ __launch_bounds__(BUCKET_THREADS) void k_integral_tree(IntegralTree tree, int level,
                                                                  unsigned long long *__restrict__ keys_out,
                                                                  mdb_integral_cell *__restrict__ values_out) {
    const uint64_t u = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    const uint64_t n = tree.n[level];
    const uint64_t first = u * BUCKET_TILE;
    if (first >= n) return;
    const uint64_t last = min(first + BUCKET_TILE, n) - 1;
    const unsigned long long *keys = tree.keys[level];
    const unsigned long long key = keys[last];
    mdb_integral_cell acc = integral_value(tree, level, last);
    for (uint64_t t = last; t > first && keys[t - 1] == key; t--) integral_cell_add(acc, integral_value(tree, level, t - 1));
    keys_out[u] = key;
    values_out[u] = acc;
}

// The lane of the last pair of each run of equal keys sums the run (its tile, then one tile's entry per level up) and
// adds it to its cell; a run without a piece leaves the cell alone.
__global__ __launch_bounds__(BUCKET_THREADS) void k_integral_fold(IntegralTree tree, mdb_integral_cell *__restrict__ cells) {
    const uint64_t j = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    const uint64_t n = tree.n[0];
    if (j >= n) return;
    const unsigned long long key = tree.keys[0][j];
    if (j + 1 < n && tree.keys[0][j + 1] == key) return;
    mdb_integral_cell acc = {0, 0.0};
    uint64_t index = j;
    for (int level = 0; level < tree.levels; level++) {
        const uint64_t first = index - index % BUCKET_TILE;
        const unsigned long long *keys = tree.keys[level];
        uint64_t t = index;
        bool whole = true; // every entry from `first` to `index` belongs to the run
        while (true) {
            if (keys[t] != key) {
                whole = false;
                break;
            }
            integral_cell_add(acc, integral_value(tree, level, t));
            if (t == first) break;
            t--;
        }
        if (!whole || first == 0) break;
        index = first / BUCKET_TILE - 1; // the tile in front, one level up
    }
    if (acc.duration == 0) return;
    mdb_integral_cell cell = cells[key];
    integral_cell_add(cell, acc);
    cells[key] = cell;
}

void integral_heads_launch(mdb_ctx *ctx, const DevSegments &s, const uint32_t *groups, const unsigned long long *offsets,
                           IntegralHead *heads, unsigned int *error) {
    LaunchTimer timer(ctx, "k_integral_heads");
    hipLaunchKernelGGL(k_integral_heads, dim3(blocks_for(s.n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, offsets,
                       heads, error);
}

static void integral_span_launch(mdb_ctx *ctx, const DevSegments &s, const uint32_t *groups, const BucketRequest &,
                                 unsigned long long *counts, unsigned int *error, const void *arg) {
    hipLaunchKernelGGL(k_integral_span, dim3(blocks_for(s.n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups,
                       *static_cast<const IntegralRequest *>(arg), counts, error);
}

// The buckets of the device batch `in` (groups: a device array or nullptr) merged into a device array of n_cells
// cells. `host_cells` (host forms): the caller's array, which is uploaded, merged into and downloaded instead; either
// way nothing of the caller's is written unless the whole call succeeds.
static int integral_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_integral_request *request,
                        uint64_t n_cells, mdb_integral_cell *dev_cells, mdb_integral_cell *host_cells) {
    const uint64_t n = in->n;
    const mdb_bucket_request &b = request->buckets;
    if (n == 0 || b.n_buckets == 0) return 0;
    const IntegralRequest q = {{b.origin, b.width, b.n_buckets, b.t_lo, b.t_hi, b.n_groups, b.which_mask},
                               request->max_gap, request->method};
    if (n > UINT64_MAX / b.n_buckets) return fail("Too many (segment, bucket) pairs for one call: split the batch.");
    const DevSegments s = to_dev(in);
    const unsigned long long *offsets = nullptr;
    unsigned int *words = nullptr;
    unsigned long long total = 0;
    const BucketSpanKernel span = {"k_integral_span", integral_span_launch, &q};
    if (bucket_span_pairs(ctx, in, s, groups, q.buckets, &offsets, &words, &total, &span)) return 1;
    if (total == 0) return 0;

    const uint64_t slice = slice_pairs_setting();
    const uint64_t n_slices = (total + slice - 1) / slice;
    const uint64_t cap = std::min<uint64_t>(slice, total);
    void *p;
    if (scratch_reserve(ctx, SCRATCH_INTEGRAL_HEADS, n * sizeof(IntegralHead), &p)) return 1;
    IntegralHead *heads = static_cast<IntegralHead *>(p);
    // Where the slices are folded: the caller's device array when nothing can fail after the first fold (one slice),
    // a working copy otherwise.
    mdb_integral_cell *cells = dev_cells;
    if (host_cells || n_slices > 1) {
        if (scratch_reserve(ctx, SCRATCH_BUCKET_CELLS, n_cells * sizeof(mdb_integral_cell), &p)) return 1;
        cells = static_cast<mdb_integral_cell *>(p);
        MDB_HIP_CHECK(hipMemcpyAsync(cells, host_cells ? host_cells : dev_cells, n_cells * sizeof(mdb_integral_cell),
                                     host_cells ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (scratch_reserve(ctx, SCRATCH_BUCKET_PAIRS, align_up(cap * sizeof(mdb_integral_cell), 256) + cap * 8, &p)) return 1;
    Carver pairs_scratch(p);
    mdb_integral_cell *partials = pairs_scratch.take<mdb_integral_cell>(cap);
    unsigned long long *keys = pairs_scratch.take<unsigned long long>(cap);
    // The tree's upper levels: ceil(n / 64) + ceil(n / 64^2) + ... entries.
    uint64_t tree_entries = 0;
    for (uint64_t m = cap; m > BUCKET_TILE;) {
        m = (m + BUCKET_TILE - 1) / BUCKET_TILE;
        tree_entries += m + 1;
    }
    if (scratch_reserve(ctx, SCRATCH_BUCKET_TREE, tree_entries * (8 + sizeof(mdb_integral_cell)) + 256, &p)) return 1;
    unsigned long long *tree_keys = static_cast<unsigned long long *>(p);
    mdb_integral_cell *tree_values = reinterpret_cast<mdb_integral_cell *>(tree_keys + tree_entries);
    const unsigned long long max_key = (unsigned long long)(n_cells - 1);
    const unsigned int key_bits = max_key == 0 ? 1u : 64u - (unsigned int)__builtin_clzll(max_key);

    // (the words are zero: bucket_span_pairs left them so; the heads' errors are read back with the first slice's)
    integral_heads_launch(ctx, s, groups, offsets, heads, words);
    for (uint64_t k = 0; k < n_slices; k++) {
        const uint64_t p0 = k * slice, p1 = std::min<uint64_t>(p0 + slice, total), m = p1 - p0;
        if (k > 0) MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
        {
            LaunchTimer timer(ctx, "k_integral_partials");
            hipLaunchKernelGGL(k_integral_partials, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, q,
                               offsets, p0, p1, heads, partials, keys, words);
        }
        bucket_keys_check(ctx, keys, m, words + 1);
        unsigned int read_back[2] = {0, 0};
        MDB_HIP_CHECK(hipMemcpyAsync(read_back, words, 8, hipMemcpyDeviceToHost, ctx->stream));
        MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        MDB_HIP_CHECK(hipGetLastError());
        if (read_back[0]) return fail(describe_error(read_back[0]));

        IntegralTree tree = {};
        tree.keys[0] = keys;
        tree.values[0] = partials;
        tree.n[0] = m;
        tree.order = nullptr;
        if (read_back[1]) { // keys out of order: a stable sort by key, pair numbers alongside
            if (bucket_keys_sort(ctx, keys, m, key_bits, &tree.keys[0], &tree.order)) return 1;
        }
        tree.levels = 1;
        uint64_t used = 0;
        {
            LaunchTimer timer(ctx, "k_integral_tree");
            for (uint64_t size = m; size > BUCKET_TILE; tree.levels++) {
                const uint64_t up = (size + BUCKET_TILE - 1) / BUCKET_TILE;
                unsigned long long *level_keys = tree_keys + used;
                mdb_integral_cell *level_values = tree_values + used;
                hipLaunchKernelGGL(k_integral_tree, dim3(blocks_for(up)), dim3(BUCKET_THREADS), 0, ctx->stream, tree,
                                   tree.levels - 1, level_keys, level_values);
                tree.keys[tree.levels] = level_keys;
                tree.values[tree.levels] = level_values;
                tree.n[tree.levels] = up;
                used += up + 1;
                size = up;
            }
        }
        {
            LaunchTimer timer(ctx, "k_integral_fold");
            hipLaunchKernelGGL(k_integral_fold, dim3(blocks_for(m)), dim3(BUCKET_THREADS), 0, ctx->stream, tree, cells);
        }
    }
    // (every slice has been found free of errors: the caller's cells are written now, and only now)
    if (host_cells)
        MDB_HIP_CHECK(hipMemcpyAsync(host_cells, cells, n_cells * sizeof(mdb_integral_cell), hipMemcpyDeviceToHost, ctx->stream));
    else if (cells != dev_cells)
        MDB_HIP_CHECK(hipMemcpyAsync(dev_cells, cells, n_cells * sizeof(mdb_integral_cell), hipMemcpyDeviceToDevice, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    return 0;
}

int integral_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                      uint32_t n_inputs, const mdb_integral_request *request, uint64_t n_cells, mdb_integral_cell *inout) {
    std::vector<uint64_t> rows(n_inputs);
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        rows[k] = inputs[k]->n;
        n += rows[k];
    }
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    // (an upload the library holds, as mdb_trend_buckets_list: the host and device forms run the same kernels)
    mdb_segments_owned *dev = nullptr;
    if (upload_segment_list_locked(ctx, inputs, n_inputs, false, &dev)) return 1;
    const uint32_t *groups = nullptr;
    int rc = upload_groups(ctx, group_of_segment, rows.data(), n_inputs, n, &groups);
    if (!rc) rc = integral_run(ctx, &dev->seg, groups, request, n_cells, nullptr, inout);
    mdb_segments_free(dev);
    return rc;
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_integral_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                                        const mdb_integral_request *request, mdb_integral_cell *inout) {
    if (!ctx || !in || !request || !inout) return fail("ctx, in, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (integral_request_check(request, &n_cells)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return integral_run(ctx, in, group_of_segment, request, n_cells, inout, nullptr);
}
