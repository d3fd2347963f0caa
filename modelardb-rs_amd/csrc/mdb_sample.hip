// mdb_sample.hip - the value of a series at regular instants, per instant and group, computed on segments
// (mdb_sample_at*): per cell the number of contributions and their f64 sum, under LINEAR (interpolate), STEP (last
// observation carried forward) or EXACT (rows on an instant only).
//
// What a caller otherwise gets from mdb_grid_batch of every point (12 B per point leaving the device), a searchsorted
// and a lerp on the host. Here a pair is (segment, instant inside the segment's extent), the extent reaching over the
// link to the right neighbour as far as the instant before the neighbour's first row, and a pair of a PMC-Mean or Swing
// segment on regular timestamps is O(1).
//
//   k_sample_span         (through bucket_span_pairs) 1 lane / segment: the instants in its extent, its group id checked.
//   k_integral_heads      (mdb_integral.hip, shared) the first row's value of each segment a link reads, 8 B / segment.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS pairs, slices folded one after the other:
//   k_sample_model_pairs  1 lane / PAIR: its segment by binary search in the pair offsets, its key, and its cell - what
//                         the model rows of a PMC-Mean or Swing segment on regular timestamps give the instant, else
//                         zero. A segment of 10^5 rows under 10^5 instants is 10^5 lanes with coalesced 16-byte stores.
//   k_sample_walk_pairs   1 lane / segment with pairs in the slice and anything left: MacaqueV values, irregular
//                         timestamps, a residual tail, the link - one walk of the rows, ADDED into the lane's own slots.
//   k_agg_bucket_check    (shared) keys non-decreasing? If not, a stable radix sort by key.
//   k_sample_tree, k_sample_fold  the one tree and fold of every per-bucket operator (mdb_bucket_fold.hpp:
//                         k_bucket_tree / k_bucket_fold<SampleFoldOps>) for a {u64, f64} partial merged with
//                         sample_cell_add: runs
//                         of equal keys reduced through the fixed tree of 64-entry tiles and merged into the cells by
//                         the lane of each run's last pair. No two lanes write one cell, no float atomics, every
//                         addition's order fixed by the pair order.
//
// Scratch: 16 B per pair (the cell) and the 8-byte key, written and read back; 8 B per segment of heads.
#include "mdb_bucket_fold.hpp"
#include "mdb_sample.hpp"
#include "mdb_scan.hpp"

#include <algorithm>

namespace mdb {

// What the tree and fold (mdb_bucket_fold.hpp) need to know of the {u64, f64} cell: merged with sample_cell_add, and a
// run without a contribution leaves its cell alone.
struct SampleFoldOps : FoldOps<mdb_sample_cell> {
    static constexpr const char *tree_name = "k_sample_tree", *fold_name = "k_sample_fold";
    __device__ __forceinline__ static mdb_sample_cell empty() { return mdb_sample_cell{0, 0.0}; }
    __device__ __forceinline__ static void merge(mdb_sample_cell &into, const mdb_sample_cell &from) { sample_cell_add(into, from); }
    __device__ __forceinline__ static bool is_empty(const mdb_sample_cell &acc) { return acc.count == 0; }
    __device__ __forceinline__ void apply(mdb_sample_cell &cell, const mdb_sample_cell &acc) const { sample_cell_add(cell, acc); }
};

__global__ __launch_bounds__(BUCKET_THREADS) void k_sample_span(DevSegments s, const uint32_t *__restrict__ groups,
                                                                SampleRequest q, unsigned long long *__restrict__ counts,
                                                                unsigned int *__restrict__ error) {
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= s.n) return;
    uint64_t first = 0;
    uint64_t count = sample_span(s, groups, i, q, &first);
    if (groups && groups[i] >= q.instants.n_groups) {
        atomicOr(error, ERR_BUCKET_GROUP);
        count = 0;
    }
    counts[i] = count;
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_sample_model_pairs(DevSegments s, const uint32_t *__restrict__ groups,
                                                                       SampleRequest q,
                                                                       const unsigned long long *__restrict__ offsets,
                                                                       uint64_t p0, uint64_t p1,
                                                                       mdb_sample_cell *__restrict__ out,
                                                                       unsigned long long *__restrict__ keys) {
    const uint64_t p = p0 + (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (p >= p1) return;
    // The segment of pair p: the last i with offsets[i] <= p (offsets[0] == 0, offsets[n] > p), in at most 64 halvings.
    uint64_t i = 0, stop = s.n;
    for (int halving = 0; halving < 64 && stop - i > 1; halving++) {
        const uint64_t middle = i + (stop - i) / 2;
        if (offsets[middle] <= p) i = middle;
        else stop = middle;
    }
    uint64_t k_first = 0;
    (void)sample_span(s, groups, i, q, &k_first);
    const uint64_t k = k_first + (p - offsets[i]);
    mdb_sample_cell cell = {0, 0.0};
    const int32_t type = s.model_type_id[i];
    if ((type == MDB_PMC_MEAN_ID || type == MDB_SWING_ID) && segment_has_regular_timestamps(s, i)) {
        const SegInfo info = analyse_segment<ANALYSE_REGULAR>(s, i);
        // (a malformed segment: k_sample_walk_pairs reports it, the call fails)
        if (!info.error && sample_closed(info.desc))
            cell = sample_model_pair(info.desc, q, sample_instant(q.instants.origin, q.instants.width, k));
    }
    keys[p - p0] = (uint64_t)(groups ? groups[i] : 0u) * q.instants.n_buckets + k;
    out[p - p0] = cell;
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_sample_walk_pairs(DevSegments s, const uint32_t *__restrict__ groups,
                                                                      SampleRequest q,
                                                                      const unsigned long long *__restrict__ offsets,
                                                                      uint64_t p0, uint64_t p1,
                                                                      const IntegralHead *__restrict__ heads,
                                                                      mdb_sample_cell *__restrict__ out,
                                                                      unsigned int *__restrict__ error_out) {
    const uint64_t i = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (i >= s.n) return;
    const uint64_t off = offsets[i], stop = offsets[i + 1];
    const uint64_t j0 = off > p0 ? off : p0, j1 = stop < p1 ? stop : p1;
    if (j0 >= j1) return;
    uint64_t k_first = 0;
    (void)sample_span(s, groups, i, q, &k_first);
    const SegInfo info = analyse_segment(s, i);
    uint32_t error = info.error;
    if (!error) {
        const bool neighbour = i + 1 < s.n && integral_same_group(groups, i, i + 1);
        sample_segment_walk(s, i, info, q, off, k_first, j0, j1, p0, out, neighbour, heads, &error);
    }
    if (error) atomicOr(error_out, error);
}

static void sample_span_launch(mdb_ctx *ctx, const DevSegments &s, const uint32_t *groups, const BucketRequest &,
                               unsigned long long *counts, unsigned int *error, const void *arg) {
    hipLaunchKernelGGL(k_sample_span, dim3(blocks_for(s.n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups,
                       *static_cast<const SampleRequest *>(arg), counts, error);
}

// The instants of the device batch `in` (groups: a device array or nullptr) merged into a device array of n_cells
// cells. `host_cells` (host forms): the caller's array, which is uploaded, merged into and downloaded instead; either
// way nothing of the caller's is written unless the whole call succeeds.
static int sample_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_sample_request *request,
                      uint64_t n_cells, mdb_sample_cell *dev_cells, mdb_sample_cell *host_cells) {
    const uint64_t n = in->n;
    const mdb_bucket_request &b = request->instants;
    if (n == 0 || b.n_buckets == 0) return 0;
    const SampleRequest q = {{b.origin, b.width, b.n_buckets, b.t_lo, b.t_hi, b.n_groups, b.which_mask},
                             request->max_gap, request->method};
    if (n > UINT64_MAX / b.n_buckets) return fail("Too many (segment, instant) pairs for one call: split the batch.");
    const DevSegments s = to_dev(in);
    const unsigned long long *offsets = nullptr;
    unsigned int *words = nullptr;
    unsigned long long total = 0;
    const BucketSpanKernel span = {"k_sample_span", sample_span_launch, &q};
    if (bucket_span_pairs(ctx, in, s, groups, q.instants, &offsets, &words, &total, &span)) return 1;
    if (total == 0) return 0;

    const uint64_t slice = slice_pairs_setting();
    const uint64_t n_slices = (total + slice - 1) / slice;
    const uint64_t cap = std::min<uint64_t>(slice, total);
    void *p;
    if (scratch_reserve(ctx, SCRATCH_INTEGRAL_HEADS, n * sizeof(IntegralHead), &p)) return 1;
    IntegralHead *heads = static_cast<IntegralHead *>(p);
    BucketCells<mdb_sample_cell> cells;
    if (cells.stage(ctx, n_cells, dev_cells, host_cells, n_slices)) return 1;
    BucketFold<SampleFoldOps> fold;
    if (fold.reserve(ctx, cap, n_cells)) return 1;
    mdb_sample_cell *partials = fold.partials();
    unsigned long long *keys = fold.keys();

    // (the words are zero: bucket_span_pairs left them so; the heads' errors are read back with the first slice's)
    if (request->method != MDB_SAMPLE_EXACT) integral_heads_launch(ctx, s, groups, offsets, heads, words);
    for (uint64_t k = 0; k < n_slices; k++) {
        const uint64_t p0 = k * slice, p1 = std::min<uint64_t>(p0 + slice, total), m = p1 - p0;
        if (k > 0) MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
        {
            LaunchTimer timer(ctx, "k_sample_model_pairs");
            hipLaunchKernelGGL(k_sample_model_pairs, dim3(blocks_for(m)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups,
                               q, offsets, p0, p1, partials, keys);
        }
        {
            LaunchTimer timer(ctx, "k_sample_walk_pairs");
            hipLaunchKernelGGL(k_sample_walk_pairs, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, q,
                               offsets, p0, p1, heads, partials, words);
        }
        unsigned int error = 0;
        bool unsorted = false;
        if (bucket_slice_check(ctx, keys, m, words, &error, &unsorted)) return 1;
        if (error) return fail(describe_error(error));
        if (fold.fold_slice(ctx, m, unsorted, cells.cells())) return 1;
    }
    return cells.commit();
}

int sample_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                    uint32_t n_inputs, const mdb_sample_request *request, uint64_t n_cells, mdb_sample_cell *inout) {
    // (an upload the library holds, as mdb_integral_buckets_list: the host and device forms run the same kernels)
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, false)) return 1;
    return sample_run(ctx, list.segments(), list.groups(), request, n_cells, nullptr, inout);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_sample_at_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                                 const mdb_sample_request *request, mdb_sample_cell *inout) {
    if (!ctx || !in || !request || !inout) return fail("ctx, in, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (sample_request_check(request, &n_cells)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return sample_run(ctx, in, group_of_segment, request, n_cells, inout, nullptr);
}
