// mdb_roll.hip - rolling windows over per-bucket cells on the device (mdb_roll_cells_dev): the rule of mdb_roll.hpp
// in two launches, one lane per (column, block of `window` buckets) in both.
//
//   k_roll_suffix    the lane walks its block backwards with S in registers and stores S where a window starts, to
//                    scratch laid out like the cells ([n_outer][the blocks but the last][n_inner]). Not launched when
//                    no window reads an S: stride a multiple of window (window == 1 among them), a single block.
//   k_roll_windows   the lane walks its block forward with P in registers; at every bucket that ends a window it stores
//                    the window: P itself at the block's last bucket, merge(S of the block in front, P) elsewhere.
//
// Lanes take consecutive `inner` first - for the counters of hist / dwell / transit a wave's loads of one step are 64
// adjacent 8-byte words - then consecutive blocks of one column, `window` cells apart: each lane then streams its own
// lines, a cell per step. No two lanes write one cell; no atomics; every merge is the operator's own function, in the
// order the rule states. Cells are copied as their members, 8 bytes wide where a member is (the pointers promise 8-byte
// alignment and no more).
#include "mdb_roll.hpp"

#include "mdb_common.hpp"

namespace mdb {

constexpr int ROLL_THREADS = 256;

struct RollLane {
    uint64_t outer, block, inner;
};
// Lane t of n_outer * n_blocks * n_inner: inner fastest, then the block.
__device__ __forceinline__ RollLane roll_lane(uint64_t t, uint64_t n_blocks, uint64_t n_inner) {
    const uint64_t rest = t / n_inner;
    return RollLane{rest / n_blocks, rest % n_blocks, t % n_inner};
}

template <class Ops>
__global__ __launch_bounds__(ROLL_THREADS) void k_roll_suffix(mdb_roll_request q, uint64_t n_suffix_blocks, uint64_t n_lanes,
                                                              const typename Ops::Cell *__restrict__ cells,
                                                              typename Ops::Cell *__restrict__ suffix) {
    using Cell = typename Ops::Cell;
    const uint64_t t = (uint64_t)blockIdx.x * ROLL_THREADS + threadIdx.x;
    if (t >= n_lanes) return;
    const RollLane lane = roll_lane(t, n_suffix_blocks, q.n_inner);
    const Cell *column = cells + lane.outer * q.n_buckets * q.n_inner + lane.inner;
    Cell *kept = suffix + lane.outer * (n_suffix_blocks * q.window) * q.n_inner + lane.inner;
    roll_suffix_block<Ops>(
        q, lane.block, [&](uint64_t b) { return Ops::load(column + b * q.n_inner); },
        [&](uint64_t b, const Cell &value) { Ops::store(kept + b * q.n_inner, value); });
}

template <class Ops>
__global__ __launch_bounds__(ROLL_THREADS) void k_roll_windows(mdb_roll_request q, uint64_t n_blocks, uint64_t n_suffix_blocks,
                                                               uint64_t n_windows, uint64_t n_lanes,
                                                               const typename Ops::Cell *__restrict__ cells,
                                                               const typename Ops::Cell *__restrict__ suffix,
                                                               typename Ops::Cell *__restrict__ out) {
    using Cell = typename Ops::Cell;
    const uint64_t t = (uint64_t)blockIdx.x * ROLL_THREADS + threadIdx.x;
    if (t >= n_lanes) return;
    const RollLane lane = roll_lane(t, n_blocks, q.n_inner);
    const Cell *column = cells + lane.outer * q.n_buckets * q.n_inner + lane.inner;
    const Cell *kept = suffix + lane.outer * (n_suffix_blocks * q.window) * q.n_inner + lane.inner;
    Cell *windows = out + lane.outer * n_windows * q.n_inner + lane.inner;
    roll_walk_block<Ops>(
        q, lane.block, [&](uint64_t b) { return Ops::load(column + b * q.n_inner); },
        [&](uint64_t b) { return Ops::load(kept + b * q.n_inner); },
        [&](uint64_t k, const Cell &value) { Ops::store(windows + k * q.n_inner, value); });
}

template <class Ops>
static int roll_launch(mdb_ctx *ctx, const mdb_roll_request &q, const RollPlan &plan, const RollBlocks &blocks,
                       const void *cells, void *suffix, void *out) {
    using Cell = typename Ops::Cell;
    const uint64_t columns = q.n_outer * q.n_inner;
    if (blocks.n_suffix_blocks > 0) {
        const uint64_t n_lanes = columns * blocks.n_suffix_blocks;
        LaunchTimer timer(ctx, "k_roll_suffix");
        hipLaunchKernelGGL(k_roll_suffix<Ops>, dim3((uint32_t)((n_lanes + ROLL_THREADS - 1) / ROLL_THREADS)),
                           dim3(ROLL_THREADS), 0, ctx->stream, q, blocks.n_suffix_blocks, n_lanes,
                           static_cast<const Cell *>(cells), static_cast<Cell *>(suffix));
    }
    {
        const uint64_t n_lanes = columns * blocks.n_blocks;
        LaunchTimer timer(ctx, "k_roll_windows");
        hipLaunchKernelGGL(k_roll_windows<Ops>, dim3((uint32_t)((n_lanes + ROLL_THREADS - 1) / ROLL_THREADS)),
                           dim3(ROLL_THREADS), 0, ctx->stream, q, blocks.n_blocks, blocks.n_suffix_blocks, plan.n_windows,
                           n_lanes, static_cast<const Cell *>(cells), static_cast<const Cell *>(suffix),
                           static_cast<Cell *>(out));
    }
    MDB_HIP_CHECK(hipGetLastError());
    return 0;
}

int roll_dev_run(mdb_ctx *ctx, const mdb_roll_request *request, const RollPlan *plan, const void *cells, void *out) {
    const mdb_roll_request q = *request;
    const RollBlocks blocks = roll_blocks(q);
    // (at most the cells' own count, which the plan has found to fit 64 bits with the cell size)
    const uint64_t n_lanes = q.n_outer * q.n_inner * blocks.n_blocks;
    if ((n_lanes + ROLL_THREADS - 1) / ROLL_THREADS > 0x7fffffffull)
        return fail("Too many (column, block) pairs for one launch: cut the cells by n_outer.");
    const uint64_t suffix_bytes = q.n_outer * blocks.n_suffix_blocks * q.window * q.n_inner * plan->cell_size;
    mdb::CallGuard lock(ctx);
    if (ctx->scratch_limit && suffix_bytes > ctx->scratch_limit)
        return fail("The suffix folds of " + std::to_string(q.n_outer * blocks.n_suffix_blocks) + " blocks need " +
                    std::to_string(suffix_bytes) + " bytes of scratch but the context's limit is " +
                    std::to_string(ctx->scratch_limit) + ": cut the cells by n_outer.");
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    void *suffix = nullptr;
    if (blocks.n_suffix_blocks > 0 && scratch_reserve(ctx, SCRATCH_ROLL_SUFFIX, suffix_bytes, &suffix)) return 1;
    return roll_dispatch(q.kind, [&](auto ops) {
        return roll_launch<decltype(ops)>(ctx, q, *plan, blocks, cells, suffix, out);
    });
}

} // namespace mdb
