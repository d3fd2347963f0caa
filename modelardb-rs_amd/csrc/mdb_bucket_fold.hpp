// mdb_bucket_fold.hpp - how every per-bucket operator ends: the {key, partial} pairs of one slice, keys checked to be
// non-decreasing (bucket_slice_check, mdb_buckets.hpp) or sorted, runs of equal keys reduced through a fixed tree of
// 64-entry tiles, and each run folded into its cell by the lane of the run's last pair. ONE template of the two
// kernels and of the host steps around them, for mdb_buckets.hip, mdb_m4.hip, mdb_moments.hip (and mdb_binned.hip),
// mdb_comoments.hip (and mdb_trend.hip), mdb_integral.hip, mdb_sample.hip and mdb_change.hip. Device and host code:
// included by .hip files only.
//
// What an operator says about its partial is an "ops" type:
//   using Partial, Cell            what a pair holds in scratch, and the caller's cell
//   tree_name, fold_name           the names of the two launches in mdb_profile_*
//   empty()                        the partial of no point
//   merge(Partial &, const &)      a later entry of a run added to the earlier ones'
//   is_empty(const Partial &)      a run like that leaves its cell alone
//   apply(Cell &, const Partial &) the folded run entering the cell (not static: the aggregates carry which_mask; the
//                                  object is passed to the fold kernel by value)
//   load(const Partial *), store(Partial *, const Partial &)   FoldOps' plain copies, or the operator's own words
//
//   k_bucket_tree   level l + 1 holds, per tile of level l, its last key and the fold of the run that ends the tile.
//   k_bucket_fold   1 lane / pair: the lane of a run's last pair folds the run (its tile, then one tile's entry per
//                   level up: entry `index` down to `first`, level by level) and applies it to the cell - no two lanes
//                   write one cell, no float atomics, the order of every merge fixed by the pair order.
#pragma once

#include "mdb_buckets.hpp"

#include <algorithm>

namespace mdb {

template <class P, class C = P> struct FoldOps {
    using Partial = P;
    using Cell = C;
    __device__ __forceinline__ static P load(const P *from) { return *from; }
    __device__ __forceinline__ static void store(P *to, const P &value) { *to = value; }
};

template <class P> struct FoldTree { // level 0 is the slice's pairs (keys, partials, and the sort's pair numbers); 1.. are the tree's
    const unsigned long long *keys[BUCKET_MAX_LEVELS];
    const P *values[BUCKET_MAX_LEVELS];
    uint64_t n[BUCKET_MAX_LEVELS];
    const uint32_t *order; // (level 0 in key order: values[0][order[j]]; nullptr: pair order)
    int levels;
};

template <class Ops>
__device__ __forceinline__ typename Ops::Partial fold_value(const FoldTree<typename Ops::Partial> &tree, int level,
                                                            uint64_t t) {
    return Ops::load(&tree.values[level][level == 0 && tree.order ? tree.order[t] : t]);
}

// Level `level` + 1 from `level`: per tile of BUCKET_TILE entries its last key and the fold of the run ending it.
template <class Ops>
__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_tree(FoldTree<typename Ops::Partial> tree, int level,
                                                                unsigned long long *__restrict__ keys_out,
                                                                typename Ops::Partial *__restrict__ values_out) {
    const uint64_t u = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    const uint64_t n = tree.n[level];
    const uint64_t first = u * BUCKET_TILE;
    if (first >= n) return;
    const uint64_t last = min(first + BUCKET_TILE, n) - 1;
    const unsigned long long *keys = tree.keys[level];
    const unsigned long long key = keys[last];
    typename Ops::Partial acc = fold_value<Ops>(tree, level, last);
    for (uint64_t t = last; t > first && keys[t - 1] == key; t--) Ops::merge(acc, fold_value<Ops>(tree, level, t - 1));
    keys_out[u] = key;
    Ops::store(&values_out[u], acc);
}

// The lane of the last pair of each run of equal keys folds the run and applies it to its cell; an empty run leaves
// the cell alone.
template <class Ops>
__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_fold(FoldTree<typename Ops::Partial> tree, Ops ops,
                                                                typename Ops::Cell *__restrict__ cells) {
    const uint64_t j = (uint64_t)blockIdx.x * BUCKET_THREADS + threadIdx.x;
    const uint64_t n = tree.n[0];
    if (j >= n) return;
    const unsigned long long key = tree.keys[0][j];
    if (j + 1 < n && tree.keys[0][j + 1] == key) return;
    typename Ops::Partial acc = Ops::empty();
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
            Ops::merge(acc, fold_value<Ops>(tree, level, t));
            if (t == first) break;
            t--;
        }
        if (!whole || first == 0) break;
        index = first / BUCKET_TILE - 1; // the tile in front, one level up
    }
    if (Ops::is_empty(acc)) return;
    typename Ops::Cell cell = cells[key];
    ops.apply(cell, acc);
    cells[key] = cell;
}

// The scratch of the slices and their fold. reserve(): one slice's partials and keys (SCRATCH_BUCKET_PAIRS: partials,
// then keys) and the tree's upper levels (SCRATCH_BUCKET_TREE: values, then keys - a partial may be 64-byte aligned,
// a key never needs more than 8) for slices of at most `cap` entries, and the bits of the largest key. An operator
// writes a slice to partials() / keys(), has it checked (bucket_slice_check) and folds it into `cells`.
template <class Ops> class BucketFold {
public:
    using Partial = typename Ops::Partial;
    using Cell = typename Ops::Cell;

    explicit BucketFold(const Ops &ops = Ops()) : ops_(ops) {}

    int reserve(mdb_ctx *ctx, uint64_t cap, uint64_t n_cells) {
        void *p;
        if (scratch_reserve(ctx, SCRATCH_BUCKET_PAIRS, align_up(cap * sizeof(Partial), 256) + cap * 8, &p)) return 1;
        Carver pairs_scratch(p);
        partials_ = pairs_scratch.take<Partial>(cap);
        keys_ = pairs_scratch.take<unsigned long long>(cap);
        // The tree's upper levels: ceil(n / 64) + ceil(n / 64^2) + ... entries.
        uint64_t tree_entries = 0;
        for (uint64_t m = cap; m > BUCKET_TILE;) {
            m = (m + BUCKET_TILE - 1) / BUCKET_TILE;
            tree_entries += m + 1;
        }
        if (scratch_reserve(ctx, SCRATCH_BUCKET_TREE, tree_entries * (8 + sizeof(Partial)) + 256, &p)) return 1;
        tree_values_ = static_cast<Partial *>(p);
        tree_keys_ = reinterpret_cast<unsigned long long *>(tree_values_ + tree_entries);
        const unsigned long long max_key = (unsigned long long)(n_cells - 1);
        key_bits_ = max_key == 0 ? 1u : 64u - (unsigned int)__builtin_clzll(max_key);
        return 0;
    }

    Partial *partials() const { return partials_; }
    unsigned long long *keys() const { return keys_; }

    // The slice's first m entries reduced and folded into cells[key], enqueued on the context's stream. `unsorted`:
    // what bucket_slice_check found - the keys are then sorted, stably, the pair numbers alongside.
    int fold_slice(mdb_ctx *ctx, uint64_t m, bool unsorted, Cell *cells) {
        FoldTree<Partial> tree = {};
        tree.keys[0] = keys_;
        tree.values[0] = partials_;
        tree.n[0] = m;
        tree.order = nullptr;
        if (unsorted && bucket_keys_sort(ctx, keys_, m, key_bits_, &tree.keys[0], &tree.order)) return 1;
        tree.levels = 1;
        uint64_t used = 0;
        {
            LaunchTimer timer(ctx, Ops::tree_name);
            for (uint64_t size = m; size > BUCKET_TILE; tree.levels++) {
                const uint64_t up = (size + BUCKET_TILE - 1) / BUCKET_TILE;
                unsigned long long *level_keys = tree_keys_ + used;
                Partial *level_values = tree_values_ + used;
                hipLaunchKernelGGL(k_bucket_tree<Ops>, dim3(blocks_for(up)), dim3(BUCKET_THREADS), 0, ctx->stream, tree,
                                   tree.levels - 1, level_keys, level_values);
                tree.keys[tree.levels] = level_keys;
                tree.values[tree.levels] = level_values;
                tree.n[tree.levels] = up;
                used += up + 1;
                size = up;
            }
        }
        {
            LaunchTimer timer(ctx, Ops::fold_name);
            hipLaunchKernelGGL(k_bucket_fold<Ops>, dim3(blocks_for(m)), dim3(BUCKET_THREADS), 0, ctx->stream, tree, ops_,
                               cells);
        }
        return 0;
    }

private:
    Ops ops_;
    Partial *partials_ = nullptr, *tree_values_ = nullptr;
    unsigned long long *keys_ = nullptr, *tree_keys_ = nullptr;
    unsigned int key_bits_ = 1;
};

// Where the slices are folded: the caller's device array when nothing can fail after the first fold (one slice), a
// working copy (SCRATCH_BUCKET_CELLS) for the host forms and for several slices. commit() - after every slice has been
// found free of errors - is the only place that writes the caller's cells.
template <class Cell> class BucketCells {
public:
    int stage(mdb_ctx *ctx, uint64_t n_cells, Cell *dev_cells, Cell *host_cells, uint64_t n_slices) {
        ctx_ = ctx, bytes_ = n_cells * sizeof(Cell), dev_ = dev_cells, host_ = host_cells, cells_ = dev_cells;
        if (!host_cells && n_slices <= 1) return 0;
        void *p;
        if (scratch_reserve(ctx, SCRATCH_BUCKET_CELLS, bytes_, &p)) return 1;
        cells_ = static_cast<Cell *>(p);
        MDB_HIP_CHECK(hipMemcpyAsync(cells_, host_ ? host_ : dev_, bytes_,
                                     host_ ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
    Cell *cells() const { return cells_; }
    int commit() {
        if (host_) MDB_HIP_CHECK(hipMemcpyAsync(host_, cells_, bytes_, hipMemcpyDeviceToHost, ctx_->stream));
        else if (cells_ != dev_) MDB_HIP_CHECK(hipMemcpyAsync(dev_, cells_, bytes_, hipMemcpyDeviceToDevice, ctx_->stream));
        MDB_HIP_CHECK(hipStreamSynchronize(ctx_->stream));
        MDB_HIP_CHECK(hipGetLastError());
        return 0;
    }

private:
    mdb_ctx *ctx_ = nullptr;
    uint64_t bytes_ = 0;
    Cell *dev_ = nullptr, *host_ = nullptr, *cells_ = nullptr;
};

} // namespace mdb
