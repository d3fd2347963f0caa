// mdb_roll.hpp - rolling windows over per-bucket cells (mdb_roll_*): window k of a column covers the buckets
// [k * stride, k * stride + window) of cells viewed as [n_outer][n_buckets][n_inner], and is the merge of its cells by
// the operator's own rule.
//
// Plain C++ (no HIP type): what a kind says about its cells (an "ops" type, in the spirit of mdb_bucket_fold.hpp), the
// checks of a request and the host form of the rule. It is shared by the kernels (mdb_roll.hip), by the host entry
// points (mdb_roll_host.cpp) and by the check program tests/roll_host, which runs it under the CPU sanitizers.
//
// The rule (mdb.h) is the two-scan sliding fold over blocks of m = window buckets aligned at multiples of m: P_j, the
// left-to-right folds of block j, and S_j, its right-to-left folds with the EARLIER cell as `into`. A window that starts
// at a block's first bucket is P_j[m-1]; one that starts r buckets into block j is merge(S_j[r], P_{j+1}[r-1]). Every
// window is two reads and one merge whatever m is, every cell enters two folds, and the order of every merge is fixed
// by the request alone: host and device produce the same bytes.
//
// An ops type:
//   using Cell                          the caller's cell
//   merge(Cell &into, const Cell &from) the operator's merge rule, `into` the earlier buckets
//   load(const Cell *), store(Cell *, const Cell &)   plain copies (cells are 8-byte aligned, no more)
#pragma once

#include "mdb_agg_merge.hpp"
#include "mdb_change.hpp"
#include "mdb_comoments.hpp"
#include "mdb_derived.hpp"
#include "mdb_m4.hpp"

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define MDB_ROLL_FN __host__ __device__ __forceinline__
#else
#define MDB_ROLL_FN inline
#endif

namespace mdb {

template <class C> struct RollCopies {
    using Cell = C;
    MDB_ROLL_FN static C load(const C *from) { return *from; }
    MDB_ROLL_FN static void store(C *to, const C &value) { *to = value; }
};

struct RollAggOps : RollCopies<mdb_agg_state> {
    MDB_ROLL_FN static void merge(mdb_agg_state &into, const mdb_agg_state &from) { agg_state_merge(into, from); }
};
struct RollM4Ops : RollCopies<mdb_m4_cell> {
    MDB_ROLL_FN static void merge(mdb_m4_cell &into, const mdb_m4_cell &from) { m4_merge(into, from); }
};
struct RollMomentsOps : RollCopies<mdb_moments_cell> {
    MDB_ROLL_FN static void merge(mdb_moments_cell &into, const mdb_moments_cell &from) { moments_merge(into, from); }
};
struct RollComomentsOps : RollCopies<mdb_comoments_cell> {
    MDB_ROLL_FN static void merge(mdb_comoments_cell &into, const mdb_comoments_cell &from) { comoments_merge(into, from); }
};
struct RollDerivedOps : RollCopies<mdb_derived_cell> {
    MDB_ROLL_FN static void merge(mdb_derived_cell &into, const mdb_derived_cell &from) { derived_merge(into, from); }
};
struct RollIntegralOps : RollCopies<mdb_integral_cell> {
    MDB_ROLL_FN static void merge(mdb_integral_cell &into, const mdb_integral_cell &from) { integral_cell_add(into, from); }
};
struct RollChangeOps : RollCopies<mdb_change_cell> {
    MDB_ROLL_FN static void merge(mdb_change_cell &into, const mdb_change_cell &from) { change_cell_merge(into, from); }
};
struct RollU64Ops : RollCopies<uint64_t> {
    MDB_ROLL_FN static void merge(uint64_t &into, const uint64_t &from) { into += from; }
};

static_assert(sizeof(mdb_agg_state) == 24 && sizeof(mdb_m4_cell) == 56 && sizeof(mdb_moments_cell) == 24 &&
                  sizeof(mdb_comoments_cell) == 48 && sizeof(mdb_derived_cell) == 32 && sizeof(mdb_integral_cell) == 16 &&
                  sizeof(mdb_change_cell) == 64,
              "the cell sizes of the kinds (mdb_format.h)");

// f(Ops()) for the ops type of `kind` (checked by the caller: roll_plan).
template <class F> int roll_dispatch(uint32_t kind, F &&f) {
    switch (kind) {
    case MDB_ROLL_AGG: return f(RollAggOps());
    case MDB_ROLL_M4: return f(RollM4Ops());
    case MDB_ROLL_MOMENTS: return f(RollMomentsOps());
    case MDB_ROLL_COMOMENTS: return f(RollComomentsOps());
    case MDB_ROLL_DERIVED: return f(RollDerivedOps());
    case MDB_ROLL_INTEGRAL: return f(RollIntegralOps());
    case MDB_ROLL_CHANGE: return f(RollChangeOps());
    default: return f(RollU64Ops());
    }
}

inline uint64_t roll_cell_size(uint32_t kind) {
    return (uint64_t)roll_dispatch(kind, [](auto ops) { return (int)sizeof(typename decltype(ops)::Cell); });
}

// A checked request: the counts and bytes every form needs.
struct RollPlan {
    uint64_t cell_size;
    uint64_t n_windows;  // per column
    uint64_t n_out;      // cells of out: n_outer * n_windows * n_inner
    uint64_t in_bytes, out_bytes;
    bool nothing;        // a dimension is 0 or no whole window exists: success, nothing written
};

// The checks of the request alone: kind, flags, window, stride, the overflow.
inline int roll_plan(const mdb_roll_request *q, RollPlan *plan) {
    if (q->kind > MDB_ROLL_U64)
        return fail("Unknown kind " + std::to_string(q->kind) + " in mdb_roll_request (MDB_ROLL_AGG .. MDB_ROLL_U64).");
    if (q->flags != 0) return fail("Unknown flag bits " + std::to_string(q->flags) + " in mdb_roll_request: flags must be 0.");
    if (q->window == 0) return fail("The window of mdb_roll_request must be at least 1 bucket.");
    if (q->stride == 0) return fail("The stride of mdb_roll_request must be at least 1 bucket.");
    plan->cell_size = roll_cell_size(q->kind);
    const unsigned __int128 limit = (unsigned __int128)UINT64_MAX;
    unsigned __int128 bytes = (unsigned __int128)q->n_outer * q->n_buckets;
    if (bytes <= limit) bytes *= q->n_inner;
    if (bytes <= limit) bytes *= plan->cell_size;
    if (bytes > limit) return fail("n_outer * n_buckets * n_inner * the cell size overflows 64 bits.");
    plan->in_bytes = (uint64_t)bytes;
    plan->n_windows = q->n_buckets < q->window ? 0 : (q->n_buckets - q->window) / q->stride + 1;
    plan->n_out = q->n_outer * plan->n_windows * q->n_inner; // (n_windows <= n_buckets: no overflow)
    plan->out_bytes = plan->n_out * plan->cell_size;
    plan->nothing = plan->n_out == 0;
    return 0;
}

// The checks every form makes before it reads a cell: the pointers, the request, the capacity, the overlap.
inline int roll_check(const mdb_roll_request *q, const void *cells, const void *out, uint64_t capacity_cells,
                      RollPlan *plan) {
    if (!q || !cells || !out) return fail("request, cells and out must not be NULL.");
    if (roll_plan(q, plan)) return 1;
    if (plan->nothing) return 0;
    if (capacity_cells < plan->n_out)
        return fail("capacity_cells is " + std::to_string(capacity_cells) + " but the windows need " +
                    std::to_string(plan->n_out) + " cells.");
    const uintptr_t a = reinterpret_cast<uintptr_t>(cells), b = reinterpret_cast<uintptr_t>(out);
    if ((a | b) & 7u) return fail("cells and out must be 8-byte aligned.");
    if (a < b + plan->out_bytes && b < a + plan->in_bytes) return fail("out must not overlap cells.");
    return 0;
}

// How the buckets of a checked request with windows fall into blocks.
struct RollBlocks {
    uint64_t n_blocks;         // blocks with a bucket: ceil(n_buckets / window)
    uint64_t n_suffix_blocks;  // blocks whose S a window reads: all but the last, none when stride % window == 0
};
inline RollBlocks roll_blocks(const mdb_roll_request &q) {
    RollBlocks blocks;
    blocks.n_blocks = (q.n_buckets - 1) / q.window + 1;
    blocks.n_suffix_blocks = q.stride % q.window == 0 ? 0 : blocks.n_blocks - 1;
    return blocks;
}

// The forward walk of block j of one column, for host and device: P in a register, and at every bucket that ends a
// window the window is stored - P itself at the block's last bucket, merge(S of the block in front, P) elsewhere.
// cell(b): the column's cell of bucket b; suffix(b): S of bucket b (b in the block in front); emit(k, value): window k.
template <class Ops, class CellAt, class SuffixAt, class Emit>
MDB_ROLL_FN void roll_walk_block(const mdb_roll_request &q, uint64_t j, CellAt &&cell, SuffixAt &&suffix, Emit &&emit) {
    using Cell = typename Ops::Cell;
    const uint64_t m = q.window, stride = q.stride;
    const uint64_t first = j * m;
    const uint64_t steps = q.n_buckets - first < m ? q.n_buckets - first : m;
    // The window that ends at bucket first + i starts at a = first + i + 1 - m. Block 0 holds the end of one window
    // only (a = 0, at i = m - 1): its phase is set so that it comes out 0 there.
    uint64_t phase, k;
    if (j == 0) {
        phase = (stride - (m - 1) % stride) % stride;
        k = 0;
    } else {
        const uint64_t a = first + 1 - m;
        phase = a % stride;
        k = a / stride + (phase != 0); // the first window that starts at or after a
    }
    Cell p = cell(first);
    for (uint64_t i = 0;; i++) {
        if (phase == 0 && (j > 0 || i == m - 1)) {
            if (i == m - 1) {
                emit(k, p);
            } else {
                Cell window = suffix(first + i + 1 - m);
                Ops::merge(window, p);
                emit(k, window);
            }
            k++;
        }
        if (i + 1 == steps) break;
        phase = phase + 1 == stride ? 0 : phase + 1;
        const Cell next = cell(first + i + 1);
        Ops::merge(p, next);
    }
}

// The backward walk of block j (a whole block with a block behind it): S_j[i] for i = m - 1 down to 1, kept where a
// window starts (S_j[0] is read by no window: that one is P_j[m-1]). keep(b, value): S of bucket b.
template <class Ops, class CellAt, class Keep>
MDB_ROLL_FN void roll_suffix_block(const mdb_roll_request &q, uint64_t j, CellAt &&cell, Keep &&keep) {
    using Cell = typename Ops::Cell;
    const uint64_t m = q.window, stride = q.stride;
    if (m < 2) return;
    const uint64_t first = j * m;
    uint64_t phase = (first + m - 1) % stride;
    Cell s = cell(first + m - 1);
    for (uint64_t i = m - 1;; i--) {
        if (phase == 0) keep(first + i, s);
        if (i == 1) break;
        phase = phase == 0 ? stride - 1 : phase - 1;
        Cell earlier = cell(first + i - 1);
        Ops::merge(earlier, s);
        s = earlier;
    }
}

// mdb_roll.hip: the two launches on the context's stream (everything checked, windows to write). The only step of
// mdb_roll_cells_dev that needs the device.
int roll_dev_run(mdb_ctx *ctx, const mdb_roll_request *request, const RollPlan *plan, const void *cells, void *out);

// The host form: column by column, block by block, with the S of one block in `suffix`.
template <class Ops>
int roll_host(const mdb_roll_request &q, const RollPlan &plan, const typename Ops::Cell *cells, typename Ops::Cell *out) {
    using Cell = typename Ops::Cell;
    const RollBlocks blocks = roll_blocks(q);
    std::vector<Cell> suffix(blocks.n_suffix_blocks ? q.window : 0);
    for (uint64_t outer = 0; outer < q.n_outer; outer++)
        for (uint64_t inner = 0; inner < q.n_inner; inner++) {
            const Cell *column = cells + outer * q.n_buckets * q.n_inner + inner;
            Cell *windows = out + outer * plan.n_windows * q.n_inner + inner;
            for (uint64_t j = 0; j < blocks.n_blocks; j++) {
                const uint64_t before = j == 0 ? 0 : (j - 1) * q.window;
                roll_walk_block<Ops>(
                    q, j, [&](uint64_t b) { return Ops::load(column + b * q.n_inner); },
                    [&](uint64_t b) { return suffix[b - before]; },
                    [&](uint64_t k, const Cell &value) { Ops::store(windows + k * q.n_inner, value); });
                if (j < blocks.n_suffix_blocks)
                    roll_suffix_block<Ops>(
                        q, j, [&](uint64_t b) { return Ops::load(column + b * q.n_inner); },
                        [&](uint64_t b, const Cell &value) { suffix[b - j * q.window] = value; });
            }
        }
    return 0;
}

} // namespace mdb
