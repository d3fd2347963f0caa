// mdb_change.hip - changes between consecutive points per date_bin bucket and group, computed on segments
// (mdb_change_buckets*): per cell the linked pairs whose later row lies in the bucket - how many, how many of them
// fell, the time they span, the sums of the rises, of the falls and of the values after a fall, the largest rise and
// the largest fall.
//
// What the reference can only answer with GridExec -> WindowAggExec(lag) -> AggregateExec over every rebuilt point.
// Here every step inside a PMC-Mean segment is zero - a (segment, bucket) pair is a count and a duration from row
// indices, O(1) - and a Swing segment's rows are arithmetic in registers. The pair between a segment's last point and
// its right neighbour's first belongs to the left segment, as in mdb_integral.hip, whose span, heads and linked rule
// are used as they are.
//
//   k_change_span        1 lane / segment: the buckets its extent [start_time, linked ? start_time of the next :
//                        end_time] overlaps (integral_span), its group id checked.
//   k_integral_heads     (mdb_integral.hip, shared) the first row's value of each segment a link reads, 8 B / segment.
//   then per slice of at most MDB_AGG_BUCKET_SLICE_PAIRS pairs, slices folded one after the other:
//   k_change_partials    1 lane / segment with pairs in the slice: one {key, cell} per pair (mdb_change.hpp).
//   k_agg_bucket_check   (shared) keys non-decreasing? If not, a stable radix sort by key.
//   k_change_tree, k_change_fold  the one tree and fold of every per-bucket operator (mdb_bucket_fold.hpp:
//                        k_bucket_tree / k_bucket_fold<ChangeFoldOps>) over 64-byte cells merged member by member (sums
//                        added, maxima taken), each run of equal keys merged into its cell by the lane of the run's
//                        last pair; a run that holds no linked pair (count == 0) leaves its cell alone. No two lanes
//                        write one cell, no float atomics, every addition's order fixed by the pair order.
// Every stream is one lane's: the batch's cursor index (k_*_pieces) is not used.
//
// Scratch: 64 B per pair (the cell) and the 8-byte key, written and read back; 8 B per segment of heads.
#include "mdb_bucket_fold.hpp"
#include "mdb_change.hpp"
#include "mdb_scan.hpp"

#include <algorithm>

namespace mdb {

// What the tree and fold (mdb_bucket_fold.hpp) need to know of the 64-byte cell: merged member by member, and a run
// without a linked pair leaves its cell alone.
struct ChangeFoldOps : FoldOps<mdb_change_cell> {
    static constexpr const char *tree_name = "k_change_tree", *fold_name = "k_change_fold";
    __device__ __forceinline__ static mdb_change_cell empty() { return change_cell_empty(); }
    __device__ __forceinline__ static void merge(mdb_change_cell &into, const mdb_change_cell &from) { change_cell_merge(into, from); }
    __device__ __forceinline__ static bool is_empty(const mdb_change_cell &acc) { return acc.count == 0; }
    __device__ __forceinline__ void apply(mdb_change_cell &cell, const mdb_change_cell &acc) const { change_cell_merge(cell, acc); }
};

__global__ __launch_bounds__(BUCKET_THREADS) void k_change_span(DevSegments s, const uint32_t *__restrict__ groups,
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

__global__ __launch_bounds__(BUCKET_THREADS) void k_change_partials(DevSegments s, const uint32_t *__restrict__ groups,
                                                                    IntegralRequest q,
                                                                    const unsigned long long *__restrict__ offsets,
                                                                    uint64_t p0, uint64_t p1,
                                                                    const IntegralHead *__restrict__ heads,
                                                                    mdb_change_cell *__restrict__ out,
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
        for (uint64_t j = j0; j < j1; j++) out[j - p0] = change_cell_empty(); // (the call fails)
    } else {
        const bool neighbour = i + 1 < s.n && integral_same_group(groups, i, i + 1);
        change_segment_partials(s, i, info, q, off, b_first, j0, j1, p0, out, neighbour, heads, &error);
    }
    if (error) atomicOr(error_out, error);
}

static void change_span_launch(mdb_ctx *ctx, const DevSegments &s, const uint32_t *groups, const BucketRequest &,
                               unsigned long long *counts, unsigned int *error, const void *arg) {
    hipLaunchKernelGGL(k_change_span, dim3(blocks_for(s.n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups,
                       *static_cast<const IntegralRequest *>(arg), counts, error);
}

// The buckets of the device batch `in` (groups: a device array or nullptr) merged into a device array of n_cells
// cells. `host_cells` (host forms): the caller's array, which is uploaded, merged into and downloaded instead; either
// way nothing of the caller's is written unless the whole call succeeds.
static int change_run(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const mdb_change_request *request,
                      uint64_t n_cells, mdb_change_cell *dev_cells, mdb_change_cell *host_cells) {
    const uint64_t n = in->n;
    const mdb_bucket_request &b = request->buckets;
    if (n == 0 || b.n_buckets == 0) return 0;
    // (the span and the heads are the time-weighted operator's: its request with a method nobody reads)
    const IntegralRequest q = {{b.origin, b.width, b.n_buckets, b.t_lo, b.t_hi, b.n_groups, b.which_mask},
                               request->max_gap, 0u};
    if (n > UINT64_MAX / b.n_buckets) return fail("Too many (segment, bucket) pairs for one call: split the batch.");
    const DevSegments s = to_dev(in);
    const unsigned long long *offsets = nullptr;
    unsigned int *words = nullptr;
    unsigned long long total = 0;
    const BucketSpanKernel span = {"k_change_span", change_span_launch, &q};
    if (bucket_span_pairs(ctx, in, s, groups, q.buckets, &offsets, &words, &total, &span)) return 1;
    if (total == 0) return 0;

    const uint64_t slice = slice_pairs_setting();
    const uint64_t n_slices = (total + slice - 1) / slice;
    const uint64_t cap = std::min<uint64_t>(slice, total);
    void *p;
    if (scratch_reserve(ctx, SCRATCH_INTEGRAL_HEADS, n * sizeof(IntegralHead), &p)) return 1;
    IntegralHead *heads = static_cast<IntegralHead *>(p);
    BucketCells<mdb_change_cell> cells;
    if (cells.stage(ctx, n_cells, dev_cells, host_cells, n_slices)) return 1;
    BucketFold<ChangeFoldOps> fold;
    if (fold.reserve(ctx, cap, n_cells)) return 1;
    mdb_change_cell *partials = fold.partials();
    unsigned long long *keys = fold.keys();

    // (the words are zero: bucket_span_pairs left them so; the heads' errors are read back with the first slice's)
    integral_heads_launch(ctx, s, groups, offsets, heads, words);
    for (uint64_t k = 0; k < n_slices; k++) {
        const uint64_t p0 = k * slice, p1 = std::min<uint64_t>(p0 + slice, total), m = p1 - p0;
        if (k > 0) MDB_HIP_CHECK(hipMemsetAsync(words, 0, 8, ctx->stream));
        {
            LaunchTimer timer(ctx, "k_change_partials");
            hipLaunchKernelGGL(k_change_partials, dim3(blocks_for(n)), dim3(BUCKET_THREADS), 0, ctx->stream, s, groups, q,
                               offsets, p0, p1, heads, partials, keys, words);
        }
        unsigned int error = 0;
        bool unsorted = false;
        if (bucket_slice_check(ctx, keys, m, words, &error, &unsorted)) return 1;
        if (error) return fail(describe_error(error));
        if (fold.fold_slice(ctx, m, unsorted, cells.cells())) return 1;
    }
    return cells.commit();
}

int change_list_run(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                    uint32_t n_inputs, const mdb_change_request *request, uint64_t n_cells, mdb_change_cell *inout) {
    // (an upload the library holds, as mdb_integral_buckets_list: the host and device forms run the same kernels)
    UploadedSegments list(ctx);
    if (list.upload(inputs, n_inputs, group_of_segment, false)) return 1;
    return change_run(ctx, list.segments(), list.groups(), request, n_cells, nullptr, inout);
}

} // namespace mdb

using namespace mdb;

extern "C" int mdb_change_buckets_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                                      const mdb_change_request *request, mdb_change_cell *inout) {
    if (!ctx || !in || !request || !inout) return fail("ctx, in, request and inout must not be NULL.");
    uint64_t n_cells = 0;
    if (change_request_check(request, &n_cells)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    return change_run(ctx, in, group_of_segment, request, n_cells, inout, nullptr);
}
