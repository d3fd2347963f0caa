// check_roll_host.cpp - TEST INFRASTRUCTURE: the entry points of the rolling windows that run without a GPU
// (mdb_roll_host.cpp). mdb_roll_cells is compared, byte for byte and for every kind, with the rule of mdb.h written
// out here window by window (each window folds its own S and P from the cells: O(window) merges, no sharing), on
// exactly sized heap arrays so that the sanitizers see every access past an end; uint64 windows are compared with
// plain sums; and malformed requests must fail with their messages before the device step - here a stand-in that
// counts its calls - is reached, and leave the output alone.
#include "../../modelardb-rs_amd/csrc/mdb_roll.hpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int roll_dev_run(mdb_ctx *, const mdb_roll_request *, const RollPlan *, const void *, void *) {
    device_calls++;
    return 0;
}
} // namespace mdb

using namespace mdb;

static int failures = 0;
#define CHECK(condition)                                                           \
    do {                                                                           \
        if (!(condition)) {                                                        \
            std::printf("MISMATCH line %d: %s\n", __LINE__, #condition);           \
            failures++;                                                            \
        }                                                                          \
    } while (0)

static std::mt19937_64 rng(2077);

static double some_double() {
    const double levels[] = {0.0, -0.0, 1.0, 1.0e6, -3.5};
    return levels[rng() % 5] + (double)(int64_t)(rng() % 2001 - 1000) / 512.0;
}
static float some_float() {
    const float specials[] = {0.0f, -0.0f, 1.5f, -2.25f, 1.0e6f, 3.0e38f};
    return rng() % 4 == 0 ? specials[rng() % 6] : (float)some_double();
}

// A random cell of each type; about a quarter are empty, half of those with 0xA5 in the members no merge reads.
static void fill(mdb_agg_state &c) {
    if (rng() % 4 == 0) c = mdb_agg_state{0.0, 0, FLT_MAX, -FLT_MAX};
    else c = mdb_agg_state{some_double(), (int64_t)(rng() % 1000 + 1), some_float(), some_float()};
}
template <class C> static void empty_or_garbage(C &c) {
    std::memset(&c, rng() % 2 ? 0xA5 : 0, sizeof c);
    c.count = 0;
}
static void fill(mdb_m4_cell &c) {
    if (rng() % 4 == 0) return empty_or_garbage(c);
    c = mdb_m4_cell{(int64_t)(rng() % 1000 + 1), (int64_t)(rng() % 50), (int64_t)(rng() % 50), (int64_t)(rng() % 50),
                    (int64_t)(rng() % 50), some_float(), some_float(), some_float(), some_float()};
}
static void fill(mdb_moments_cell &c) {
    if (rng() % 4 == 0) return empty_or_garbage(c);
    c = mdb_moments_cell{(int64_t)(rng() % 1000 + 1), some_double(), std::fabs(some_double())};
}
static void fill(mdb_comoments_cell &c) {
    if (rng() % 4 == 0) return empty_or_garbage(c);
    c = mdb_comoments_cell{(int64_t)(rng() % 1000 + 1), some_double(), some_double(), std::fabs(some_double()),
                           std::fabs(some_double()), some_double()};
}
static void fill(mdb_derived_cell &c) {
    if (rng() % 4 == 0) return empty_or_garbage(c);
    c = mdb_derived_cell{(int64_t)(rng() % 1000 + 1), some_double(), std::fabs(some_double()), some_float(), some_float()};
}
static void fill(mdb_integral_cell &c) { c = mdb_integral_cell{rng() % 4 ? rng() >> 8 : 0, some_double()}; }
static void fill(mdb_change_cell &c) {
    c = mdb_change_cell{rng() % 1000, rng() % 100, rng() >> 8, std::fabs(some_double()), std::fabs(some_double()),
                        some_double(), std::fabs(some_double()), std::fabs(some_double())};
    if (rng() % 4 == 0) std::memset(&c, 0, sizeof c);
}
static void fill(uint64_t &c) { c = rng() % 2 ? rng() : rng() >> 30; }

// The rule of mdb.h for ONE window, from the cells alone.
template <class Ops>
static typename Ops::Cell window_by_the_rule(const typename Ops::Cell *column, uint64_t n_inner, uint64_t a, uint64_t m) {
    using Cell = typename Ops::Cell;
    auto at = [&](uint64_t b) { return column[b * n_inner]; };
    const uint64_t j = a / m, r = a % m;
    if (r == 0) {
        Cell p = at(j * m);
        for (uint64_t i = 1; i < m; i++) Ops::merge(p, at(j * m + i));
        return p;
    }
    Cell s = at(j * m + m - 1);
    for (uint64_t i = m - 1; i > r; i--) {
        Cell earlier = at(j * m + i - 1);
        Ops::merge(earlier, s);
        s = earlier;
    }
    Cell p = at((j + 1) * m);
    for (uint64_t i = 1; i < r; i++) Ops::merge(p, at((j + 1) * m + i));
    Ops::merge(s, p);
    return s;
}

template <class Ops> static void check_kind(uint32_t kind, uint64_t *compared) {
    using Cell = typename Ops::Cell;
    const uint64_t windows[] = {1, 2, 3, 7, 64, 65};
    for (uint64_t m : windows)
        for (uint64_t n_buckets : {m, m + 1, 2 * m - 1, (uint64_t)150})
            for (uint64_t stride : {(uint64_t)1, (uint64_t)2, m, m + 1})
                for (uint64_t n_inner : {(uint64_t)1, (uint64_t)3}) {
                    if (n_buckets < m) continue;
                    const uint64_t n_outer = 2;
                    const mdb_roll_request q = {kind, 0, n_outer, n_buckets, n_inner, m, stride};
                    uint64_t n_windows = 0;
                    CHECK(mdb_roll_windows(&q, &n_windows) == 0 && n_windows == (n_buckets - m) / stride + 1);
                    std::vector<Cell> cells(n_outer * n_buckets * n_inner), out(n_outer * n_windows * n_inner);
                    for (Cell &c : cells) fill(c);
                    std::memset(out.data(), 0x5A, out.size() * sizeof(Cell));
                    const std::vector<Cell> before = cells;
                    CHECK(mdb_roll_cells(&q, cells.data(), out.data(), out.size()) == 0);
                    CHECK(std::memcmp(cells.data(), before.data(), cells.size() * sizeof(Cell)) == 0);
                    for (uint64_t outer = 0; outer < n_outer; outer++)
                        for (uint64_t k = 0; k < n_windows; k++)
                            for (uint64_t inner = 0; inner < n_inner; inner++) {
                                const Cell expected = window_by_the_rule<Ops>(cells.data() + outer * n_buckets * n_inner + inner,
                                                                              n_inner, k * stride, m);
                                const Cell &got = out[(outer * n_windows + k) * n_inner + inner];
                                if (std::memcmp(&got, &expected, sizeof(Cell)) != 0) {
                                    std::printf("kind %u window %llu stride %llu buckets %llu inner %llu: window %llu differs\n", kind,
                                                (unsigned long long)m, (unsigned long long)stride, (unsigned long long)n_buckets,
                                                (unsigned long long)n_inner, (unsigned long long)k);
                                    CHECK(false);
                                }
                                ++*compared;
                            }
                }
}

static void check_sums() {
    const uint64_t n_buckets = 1000, n_inner = 5;
    std::vector<uint64_t> cells(n_buckets * n_inner);
    for (uint64_t &c : cells) c = rng();
    for (uint64_t m : {(uint64_t)1, (uint64_t)60, (uint64_t)999, (uint64_t)1000})
        for (uint64_t stride : {(uint64_t)1, (uint64_t)7, (uint64_t)60}) {
            const mdb_roll_request q = {MDB_ROLL_U64, 0, 1, n_buckets, n_inner, m, stride};
            uint64_t n_windows = 0;
            CHECK(mdb_roll_windows(&q, &n_windows) == 0);
            std::vector<uint64_t> out(n_windows * n_inner);
            CHECK(mdb_roll_cells(&q, cells.data(), out.data(), out.size()) == 0);
            for (uint64_t k = 0; k < n_windows; k++)
                for (uint64_t inner = 0; inner < n_inner; inner++) {
                    uint64_t sum = 0;
                    for (uint64_t b = k * stride; b < k * stride + m; b++) sum += cells[b * n_inner + inner];
                    CHECK(out[k * n_inner + inner] == sum);
                }
        }
}

static bool said(const char *word) { return g_last_error.find(word) != std::string::npos; }

static void check_requests() {
    mdb_ctx *fake = reinterpret_cast<mdb_ctx *>(8); // (never dereferenced)
    std::vector<mdb_moments_cell> cells(40), out(40);
    std::memset(out.data(), 0xA5, 40 * sizeof(mdb_moments_cell));
    const std::vector<mdb_moments_cell> before = out;
    const mdb_roll_request ok = {MDB_ROLL_MOMENTS, 0, 2, 10, 1, 3, 1};
    struct Wrong {
        mdb_roll_request q;
        const void *cells;
        void *out;
        uint64_t capacity;
        const char *word;
    };
    const Wrong wrong[] = {
        {{8, 0, 2, 10, 1, 3, 1}, cells.data(), out.data(), 40, "kind"},
        {{MDB_ROLL_MOMENTS, 2, 2, 10, 1, 3, 1}, cells.data(), out.data(), 40, "flag"},
        {{MDB_ROLL_MOMENTS, 0, 2, 10, 1, 0, 1}, cells.data(), out.data(), 40, "window"},
        {{MDB_ROLL_MOMENTS, 0, 2, 10, 1, 3, 0}, cells.data(), out.data(), 40, "stride"},
        {{MDB_ROLL_MOMENTS, 0, 1ull << 40, 1ull << 30, 1, 3, 1}, cells.data(), out.data(), 40, "overflows"},
        {{MDB_ROLL_MOMENTS, 0, 1ull << 61, 1, 1, 1, 1}, cells.data(), out.data(), 40, "overflows"},
        {{MDB_ROLL_U64, 0, UINT64_MAX, UINT64_MAX, UINT64_MAX, 1, 1}, cells.data(), out.data(), 40, "overflows"},
        {ok, cells.data(), out.data(), 15, "16 cells"},
        {ok, cells.data(), cells.data() + 5, 40, "overlap"},
        {ok, cells.data(), reinterpret_cast<char *>(out.data()) + 4, 40, "aligned"},
        {ok, nullptr, out.data(), 40, "NULL"},
        {ok, cells.data(), nullptr, 40, "NULL"},
    };
    for (const Wrong &w : wrong) {
        CHECK(mdb_roll_cells(&w.q, w.cells, w.out, w.capacity) == 1 && said(w.word));
        CHECK(mdb_roll_cells_dev(fake, &w.q, w.cells, w.out, w.capacity) == 1 && said(w.word));
    }
    CHECK(mdb_roll_cells(nullptr, cells.data(), out.data(), 40) == 1 && said("NULL"));
    CHECK(mdb_roll_cells_dev(nullptr, &ok, cells.data(), out.data(), 40) == 1 && said("NULL"));
    uint64_t n_windows = 99;
    CHECK(mdb_roll_windows(nullptr, &n_windows) == 1 && mdb_roll_windows(&ok, nullptr) == 1 && n_windows == 99);
    // the empty cases succeed without the device
    const mdb_roll_request empties[] = {{MDB_ROLL_MOMENTS, 0, 0, 10, 1, 3, 1}, {MDB_ROLL_MOMENTS, 0, 2, 0, 1, 3, 1},
                                        {MDB_ROLL_MOMENTS, 0, 2, 10, 0, 3, 1}, {MDB_ROLL_MOMENTS, 0, 2, 2, 1, 3, 1}};
    for (const mdb_roll_request &q : empties) {
        CHECK(mdb_roll_cells(&q, cells.data(), out.data(), 0) == 0);
        CHECK(mdb_roll_cells_dev(fake, &q, cells.data(), out.data(), 0) == 0);
        CHECK(mdb_roll_windows(&q, &n_windows) == 0 && (n_windows == 0 || q.n_outer == 0 || q.n_inner == 0));
    }
    CHECK(device_calls == 0);
    CHECK(std::memcmp(out.data(), before.data(), 40 * sizeof(mdb_moments_cell)) == 0);
    // and a good call reaches the device step
    CHECK(mdb_roll_cells_dev(fake, &ok, cells.data(), out.data(), 16) == 0 && device_calls == 1);
    // the largest counts that do not overflow
    const mdb_roll_request huge = {MDB_ROLL_U64, 0, 1, UINT64_MAX / 8, 1, 60, 60};
    CHECK(mdb_roll_windows(&huge, &n_windows) == 0 && n_windows == (UINT64_MAX / 8 - 60) / 60 + 1);
}

int main() {
    uint64_t compared = 0;
    check_kind<RollAggOps>(MDB_ROLL_AGG, &compared);
    check_kind<RollM4Ops>(MDB_ROLL_M4, &compared);
    check_kind<RollMomentsOps>(MDB_ROLL_MOMENTS, &compared);
    check_kind<RollComomentsOps>(MDB_ROLL_COMOMENTS, &compared);
    check_kind<RollDerivedOps>(MDB_ROLL_DERIVED, &compared);
    check_kind<RollIntegralOps>(MDB_ROLL_INTEGRAL, &compared);
    check_kind<RollChangeOps>(MDB_ROLL_CHANGE, &compared);
    check_kind<RollU64Ops>(MDB_ROLL_U64, &compared);
    check_sums();
    check_requests();
    if (failures) {
        std::printf("%d MISMATCH(es)\n", failures);
        return 1;
    }
    std::printf("ok: %llu windows of eight kinds by the rule, the sums and the checks of the rolling windows\n",
                (unsigned long long)compared);
    return 0;
}
