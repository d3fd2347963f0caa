// mdb_hist.hpp - the host arithmetic of the value histograms and exact quantiles (mdb_hist_*, mdb_quantile_*): the
// edges' validation and the cell rule, the ranks of a quantile, and the refinement that pins an order statistic with
// three histogram passes. No device code and no HIP type: mdb_hist.hip runs the passes on the segments, and the
// check program tests/hist_host/check_hist_host.cpp drives the same code under the CPU sanitizers with a pass made of
// a sorted array.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mdb_host_side.hpp"

namespace mdb {

// total_order_key of mdb_filter.hpp for host code without HIP, and its inverse: the map is an involution on the 32
// bits, so EVERY key is the key of exactly one f32 bit pattern and an edge at any key is an exact float.
inline int32_t hist_key_of_bits(uint32_t bits) { return (int32_t)(bits ^ ((uint32_t)((int32_t)bits >> 31) & 0x7fffffffu)); }
inline uint32_t hist_bits_of_key(int32_t key) { return (uint32_t)key ^ ((uint32_t)(key >> 31) & 0x7fffffffu); }
inline int32_t hist_key_of(float value) {
    uint32_t bits;
    std::memcpy(&bits, &value, 4);
    return hist_key_of_bits(bits);
}
inline float hist_float_of_key(int32_t key) {
    const uint32_t bits = hist_bits_of_key(key);
    float value;
    std::memcpy(&value, &bits, 4);
    return value;
}

// The edges of a histogram as keys: 1 .. MDB_HIST_MAX_EDGES of them, strictly increasing in totalOrder.
inline int hist_edge_keys(const float *edges, uint32_t n_edges, std::vector<int32_t> *keys) {
    if (!edges) return fail("edges must not be NULL.");
    if (n_edges < 1 || n_edges > MDB_HIST_MAX_EDGES)
        return fail("n_edges must be 1 .. " + std::to_string(MDB_HIST_MAX_EDGES) + ".");
    keys->resize(n_edges);
    for (uint32_t j = 0; j < n_edges; j++) {
        (*keys)[j] = hist_key_of(edges[j]);
        if (j > 0 && (*keys)[j] <= (*keys)[j - 1])
            return fail("The edges must be strictly increasing in totalOrder (edge " + std::to_string(j) + " is not above edge " +
                        std::to_string(j - 1) + ").");
    }
    return 0;
}

// The cell of a key: the number of edges at or below it.
inline uint32_t hist_cell_of_key(const std::vector<int32_t> &edge_keys, int32_t key) {
    return (uint32_t)(std::upper_bound(edge_keys.begin(), edge_keys.end(), key) - edge_keys.begin());
}

// p = q * (N - 1) in f64: the ranks floor(p) and ceil(p) (0-based, at most N - 1) and p - floor(p).
inline int quantile_ranks(double q, uint64_t n_points, uint64_t *rank_lo, uint64_t *rank_hi, double *fraction) {
    if (n_points == 0) return fail("A quantile needs at least one point.");
    if (!(q >= 0.0 && q <= 1.0)) return fail("q must lie in [0, 1].");
    const double p = q * (double)(n_points - 1);
    const double below = std::floor(p), above = std::ceil(p);
    // ((double)(N - 1) may round up beyond 2^53: no rank lies past the last point)
    const uint64_t last = n_points - 1;
    *rank_lo = below >= 18446744073709551616.0 ? last : std::min<uint64_t>((uint64_t)below, last);
    *rank_hi = above >= 18446744073709551616.0 ? last : std::min<uint64_t>((uint64_t)above, last);
    *fraction = p - below;
    return 0;
}

// ---- refinement: an order statistic from histogram passes ---------------------------------------------------------
// The 2^32 keys are cut 12 + 12 + 8 bits deep: pass 1 has 4 095 edges 2^20 keys apart over the whole key space, pass 2
// has 4 095 edges 2^8 keys apart inside the cell of pass 1 that holds the rank, pass 3 has 255 edges one key apart
// inside the cell of pass 2 - its cells are single keys. Cell 0 of a later pass also holds every point below the range
// it refines and its last cell every point above, so the rank looked for stays the rank among ALL points: the cell
// that holds rank r is the first whose running count exceeds r, in every pass.

constexpr uint32_t QUANTILE_MAX_Q = 16;

// The edges of a pass over the keys [first, first + (n_cells << shift)), n_cells cells of 1 << shift keys each.
inline void quantile_pass_edges(int64_t first, uint32_t shift, uint32_t n_cells, std::vector<float> *edges) {
    edges->resize(n_cells - 1);
    for (uint32_t j = 1; j < n_cells; j++) (*edges)[j - 1] = hist_float_of_key((int32_t)(first + ((int64_t)j << shift)));
}

// The first cell whose running count exceeds `rank` (rank below the sum of the counts).
inline uint32_t quantile_cell_of_rank(const std::vector<uint64_t> &counts, uint64_t rank) {
    uint64_t running = 0;
    for (uint32_t c = 0; c < counts.size(); c++) {
        running += counts[c];
        if (running > rank) return c;
    }
    return (uint32_t)counts.size() - 1;
}

// `pass(edges, n_edges, counts)`: a fresh histogram of all points under the n_edges edges into counts[n_edges + 1]
// (0, or 1 with the error set). Ranks of the n_q quantiles q[i] -> out_lo[i] / out_hi[i]; *n_points the number of
// points, found by the first pass (0: nothing else is written). *n_passes (may be nullptr): the passes run.
template <typename Pass>
int quantile_refine(const double *q, uint32_t n_q, Pass &&pass, float *out_lo, float *out_hi, uint64_t *n_points,
                    uint32_t *n_passes) {
    uint32_t passes = 0;
    std::vector<float> edges;
    auto run = [&](int64_t first, uint32_t shift, uint32_t n_cells, std::vector<uint64_t> *counts) {
        quantile_pass_edges(first, shift, n_cells, &edges);
        counts->assign(n_cells, 0);
        passes += 1;
        return pass(edges.data(), n_cells - 1, counts->data());
    };
    std::vector<uint64_t> top, middle, bottom;
    if (run((int64_t)INT32_MIN, 20, 4096, &top)) return 1;
    uint64_t total = 0;
    for (uint64_t c : top) total += c;
    if (n_passes) *n_passes = passes;
    if (total == 0) {
        *n_points = 0;
        return 0;
    }
    // The distinct ranks, in order: neighbours share their passes whenever they share a cell.
    std::vector<uint64_t> ranks(2 * (size_t)n_q);
    for (uint32_t i = 0; i < n_q; i++) {
        double fraction;
        if (quantile_ranks(q[i], total, &ranks[2 * i], &ranks[2 * i + 1], &fraction)) return 1;
    }
    std::vector<uint64_t> distinct = ranks;
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    std::vector<int32_t> key_of_rank(distinct.size());
    uint32_t top_cell = UINT32_MAX, middle_cell = UINT32_MAX;
    int64_t middle_first = 0, bottom_first = 0;
    for (size_t k = 0; k < distinct.size(); k++) {
        const uint32_t c1 = quantile_cell_of_rank(top, distinct[k]);
        if (c1 != top_cell) {
            middle_first = (int64_t)INT32_MIN + ((int64_t)c1 << 20);
            if (run(middle_first, 8, 4096, &middle)) return 1;
            top_cell = c1;
            middle_cell = UINT32_MAX;
        }
        const uint32_t c2 = quantile_cell_of_rank(middle, distinct[k]);
        if (c2 != middle_cell) {
            bottom_first = middle_first + ((int64_t)c2 << 8);
            if (run(bottom_first, 0, 256, &bottom)) return 1;
            middle_cell = c2;
        }
        key_of_rank[k] = (int32_t)(bottom_first + (int64_t)quantile_cell_of_rank(bottom, distinct[k]));
    }
    auto value_of = [&](uint64_t rank) {
        const size_t k = (size_t)(std::lower_bound(distinct.begin(), distinct.end(), rank) - distinct.begin());
        return hist_float_of_key(key_of_rank[k]);
    };
    for (uint32_t i = 0; i < n_q; i++) {
        out_lo[i] = value_of(ranks[2 * i]);
        out_hi[i] = value_of(ranks[2 * i + 1]);
    }
    *n_points = total;
    if (n_passes) *n_passes = passes;
    return 0;
}

// What every quantile call checks before it touches the device.
inline int quantile_arguments_check(const double *q, uint32_t n_q) {
    if (n_q < 1 || n_q > QUANTILE_MAX_Q) return fail("n_q must be 1 .. " + std::to_string(QUANTILE_MAX_Q) + ".");
    for (uint32_t i = 0; i < n_q; i++)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail("q must lie in [0, 1].");
    return 0;
}

} // namespace mdb
