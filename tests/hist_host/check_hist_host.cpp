// check_hist_host.cpp - TEST INFRASTRUCTURE: mdb_hist.hpp without a GPU. The histogram pass the refinement asks for is
// answered from a plain array of keys (the cell rule applied point by point), so that quantile_refine, its edge
// generation, the edges' validation, the cell rule and the ranks run under the CPU sanitizers; every order statistic is
// compared with the sorted array's.
#include "../../modelardb-rs_amd/csrc/mdb_hist.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

namespace mdb {
thread_local std::string g_last_error;
}

using namespace mdb;

static int failures = 0;
#define CHECK(condition)                                                           \
    do {                                                                           \
        if (!(condition)) {                                                        \
            std::printf("MISMATCH line %d: %s\n", __LINE__, #condition);           \
            failures++;                                                            \
        }                                                                          \
    } while (0)

static float from_bits(uint32_t bits) {
    float v;
    std::memcpy(&v, &bits, 4);
    return v;
}
static uint32_t bits_of(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    return bits;
}

// The refinement over `keys` (any order), against the sorted keys.
static uint32_t check_quantiles(std::vector<int32_t> keys, const std::vector<double> &q) {
    uint32_t passes = 0;
    auto pass = [&](const float *edges, uint32_t n_edges, uint64_t *counts) {
        std::vector<int32_t> edge_keys;
        if (hist_edge_keys(edges, n_edges, &edge_keys)) return 1;
        for (int32_t key : keys) counts[hist_cell_of_key(edge_keys, key)] += 1;
        return 0;
    };
    std::vector<float> lo(q.size(), from_bits(0x12345678u)), hi(q.size(), from_bits(0x12345678u));
    uint64_t n_points = 77;
    CHECK(quantile_refine(q.data(), (uint32_t)q.size(), pass, lo.data(), hi.data(), &n_points, &passes) == 0);
    CHECK(n_points == keys.size());
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < q.size(); i++) {
        if (keys.empty()) {
            CHECK(bits_of(lo[i]) == 0x12345678u && bits_of(hi[i]) == 0x12345678u);
            continue;
        }
        uint64_t rank_lo, rank_hi;
        double fraction;
        CHECK(quantile_ranks(q[i], keys.size(), &rank_lo, &rank_hi, &fraction) == 0);
        CHECK(bits_of(lo[i]) == hist_bits_of_key(keys[rank_lo]));
        CHECK(bits_of(hi[i]) == hist_bits_of_key(keys[rank_hi]));
    }
    return passes;
}

int main() {
    // the key map: an involution, monotone along totalOrder
    const uint32_t ordered[] = {0xffffffffu, 0xffc00000u, 0xff800000u, 0xff7fffffu, 0xbf800000u, 0x80000001u, 0x80000000u,
                                0x00000000u, 0x00000001u, 0x3f800000u, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u, 0x7fffffffu};
    for (size_t k = 0; k < sizeof(ordered) / 4; k++) {
        CHECK(hist_bits_of_key(hist_key_of_bits(ordered[k])) == ordered[k]);
        if (k > 0) CHECK(hist_key_of_bits(ordered[k - 1]) < hist_key_of_bits(ordered[k]));
    }
    CHECK(hist_key_of_bits(0xffffffffu) == INT32_MIN && hist_key_of_bits(0x7fffffffu) == INT32_MAX);

    // edges: validation and the cell rule
    std::vector<int32_t> keys;
    const float good[] = {from_bits(0xff800000u), -1.0f, from_bits(0x80000000u), 0.0f, 1.0f, from_bits(0x7fc00000u)};
    CHECK(hist_edge_keys(good, 6, &keys) == 0 && keys.size() == 6);
    for (size_t k = 0; k < sizeof(ordered) / 4; k++) {
        uint32_t expected = 0;
        for (float e : good) expected += hist_key_of(e) <= hist_key_of_bits(ordered[k]);
        CHECK(hist_cell_of_key(keys, hist_key_of_bits(ordered[k])) == expected);
    }
    const float equal[] = {1.0f, 1.0f}, descending[] = {2.0f, 1.0f}, zeros[] = {0.0f, from_bits(0x80000000u)};
    CHECK(hist_edge_keys(equal, 2, &keys) == 1 && hist_edge_keys(descending, 2, &keys) == 1 && hist_edge_keys(zeros, 2, &keys) == 1);
    CHECK(hist_edge_keys(good, 0, &keys) == 1 && hist_edge_keys(nullptr, 1, &keys) == 1);
    std::vector<float> many(MDB_HIST_MAX_EDGES + 1);
    for (size_t j = 0; j < many.size(); j++) many[j] = (float)j;
    CHECK(hist_edge_keys(many.data(), MDB_HIST_MAX_EDGES + 1, &keys) == 1);
    CHECK(hist_edge_keys(many.data(), MDB_HIST_MAX_EDGES, &keys) == 0 && keys.size() == MDB_HIST_MAX_EDGES);

    // the edges of the three passes: strictly increasing, exact, the right distance apart
    std::vector<float> edges;
    const int64_t firsts[] = {(int64_t)INT32_MIN, (int64_t)INT32_MIN + (4095ll << 20), -(1ll << 20), 0};
    for (int64_t first : firsts) {
        const uint32_t shifts[] = {20, 8, 0};
        const uint32_t cells[] = {4096, 4096, 256};
        for (int level = (first == (int64_t)INT32_MIN ? 0 : 1); level < 3; level++) {
            quantile_pass_edges(first, shifts[level], cells[level], &edges);
            CHECK(edges.size() == cells[level] - 1);
            CHECK(hist_edge_keys(edges.data(), (uint32_t)edges.size(), &keys) == 0);
            for (size_t j = 0; j < keys.size(); j++) CHECK((int64_t)keys[j] == first + ((int64_t)(j + 1) << shifts[level]));
        }
    }

    // ranks
    uint64_t lo, hi;
    double fraction;
    CHECK(quantile_ranks(0.5, 0, &lo, &hi, &fraction) == 1 && quantile_ranks(-0.1, 5, &lo, &hi, &fraction) == 1);
    CHECK(quantile_ranks(1.5, 5, &lo, &hi, &fraction) == 1 && quantile_ranks(std::nan(""), 5, &lo, &hi, &fraction) == 1);
    CHECK(quantile_ranks(0.5, 4, &lo, &hi, &fraction) == 0 && lo == 1 && hi == 2 && fraction == 0.5);
    CHECK(quantile_ranks(1.0, UINT64_MAX, &lo, &hi, &fraction) == 0 && lo == UINT64_MAX - 1 && hi == UINT64_MAX - 1);
    CHECK(quantile_ranks(1.0, (1ull << 53) + 2, &lo, &hi, &fraction) == 0 && hi <= (1ull << 53) + 1);
    const double bad_q[] = {0.5, 2.0};
    CHECK(quantile_arguments_check(bad_q, 2) == 1 && quantile_arguments_check(bad_q, 0) == 1 && quantile_arguments_check(bad_q, 17) == 1);
    CHECK(quantile_arguments_check(bad_q, 1) == 0);

    // the refinement
    const std::vector<double> five = {0.0, 0.25, 0.5, 0.999, 1.0};
    std::vector<double> sixteen;
    for (int k = 0; k < 16; k++) sixteen.push_back(k / 15.0);
    std::mt19937_64 rng(20261018);
    uint32_t most_passes = 0;
    CHECK(check_quantiles({}, five) == 1);
    CHECK(check_quantiles({hist_key_of(37.0f)}, five) == 3);
    CHECK(check_quantiles(std::vector<int32_t>(1000, hist_key_of(5.0f)), sixteen) == 3);
    CHECK(check_quantiles({INT32_MIN, INT32_MAX}, five) == 5);
    CHECK(check_quantiles({INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, 0, -1}, sixteen) >= 3);
    for (int trial = 0; trial < 40; trial++) {
        const size_t n = 1 + (size_t)(rng() % 3000);
        std::vector<int32_t> sample(n);
        for (auto &key : sample) {
            switch (rng() % 6) {
            case 0: key = (int32_t)(uint32_t)rng(); break;                                   // anywhere, NaNs included
            case 1: key = hist_key_of(100.0f + (float)(rng() % 1000) * 0.01f); break;         // a narrow band
            case 2: key = hist_key_of(trial % 2 ? 0.0f : from_bits(0x80000000u)); break;      // zeros
            case 3: key = hist_key_of((float)(int)(rng() % 7) - 3.0f); break;                 // many repeats
            case 4: key = hist_key_of(from_bits(0x7fc00000u | (uint32_t)(rng() % 3))); break; // NaNs
            default: key = hist_key_of(-1e30f * (float)(rng() % 100)); break;
            }
        }
        most_passes = std::max(most_passes, check_quantiles(sample, trial % 2 ? five : sixteen));
    }
    CHECK(most_passes <= 1 + 2 * 32);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok: the host arithmetic of the histograms and quantiles (at most %u passes per call)\n", most_passes);
    return 0;
}
