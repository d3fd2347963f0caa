// check_transit_host.cpp - TEST INFRASTRUCTURE: the part of the transitions operator that needs no GPU. The walk of a
// run of rows (transit_walk_point of mdb_transit.hpp) is compared with a pair-by-pair evaluation in 128-bit integers,
// also under the far bucket requests (origin INT64_MIN, width INT64_MAX), equal and backward timestamps; the row ranges
// the kernel's closed forms rest on (change_regular_rows) are compared with the walk; mdb_transit_merge_n and
// mdb_transit_crossings are checked on counters; and the host forms (mdb_transit_host.cpp) are handed malformed
// requests and edge lists: they must fail with their messages before transit_list_run - here a stand-in that counts
// its calls - is reached, and leave the counters alone.
#include "../../modelardb-rs_amd/csrc/mdb_transit.hpp"

#include <climits>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int transit_list_run(mdb_ctx *, const mdb_segments *const *, const uint32_t *const *, uint32_t, const mdb_transit_request *,
                     const std::vector<int32_t> &, uint64_t, uint64_t *) {
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

struct Point {
    int64_t t;
    int32_t key;
};

using Pairs = std::map<std::tuple<uint64_t, int32_t, int32_t>, uint64_t>; // (bucket, from key, to key) -> pairs

// Pair by pair, the later row's bucket in 128-bit integers (nothing wraps or saturates here).
static Pairs reference_pairs(const std::vector<Point> &points, int64_t max_gap, int64_t origin, int64_t width, uint64_t b0,
                             uint64_t b1) {
    Pairs pairs;
    for (size_t k = 0; k + 1 < points.size(); k++) {
        const __int128 t0 = points[k].t, t1 = points[k + 1].t;
        if (t1 <= t0 || t1 - t0 > (__int128)max_gap || t1 < (__int128)origin) continue;
        const __int128 b = (t1 - (__int128)origin) / width;
        if (b >= (__int128)b0 && b < (__int128)b1) pairs[{(uint64_t)b, points[k].key, points[k + 1].key}] += 1;
    }
    return pairs;
}

static Pairs walk_pairs(const std::vector<Point> &points, int64_t max_gap, int64_t origin, int64_t width, uint64_t b0,
                        uint64_t b1) {
    Pairs pairs;
    const TransitWindow w = {origin, width, max_gap, b0, b1};
    TransitWalk walk = transit_walk_start();
    for (const Point &p : points)
        transit_walk_point(w, walk, p.t, p.key, [&](uint64_t b, int32_t from, int32_t to) {
            CHECK(b >= b0 && b < b1);
            pairs[{b, from, to}] += 1;
        });
    return pairs;
}

// A run of n rows start + k * delta with keys key_at(k): the walk against the reference in every bucket of [b0, b1),
// and, where the gap rule links the rows, the later rows change_regular_rows gives per bucket against both.
template <typename KeyAt>
static void check_run(const char *name, int64_t start, int64_t delta, uint32_t n, KeyAt key_at, int64_t origin, int64_t width,
                      uint64_t b0, uint64_t b1, int64_t max_gap) {
    std::vector<Point> points;
    for (uint32_t k = 0; k < n; k++) points.push_back(Point{(int64_t)((uint64_t)start + (uint64_t)k * (uint64_t)delta), key_at(k)});
    const Pairs expected = reference_pairs(points, max_gap, origin, width, b0, b1);
    const Pairs walked = walk_pairs(points, max_gap, origin, width, b0, b1);
    if (walked != expected) {
        std::printf("MISMATCH %s: the walk gives %zu counters, the reference %zu\n", name, walked.size(), expected.size());
        failures++;
    }
    if (!integral_linked(max_gap, 0, delta)) {
        CHECK(expected.empty());
        return;
    }
    Pairs closed;
    for (uint64_t b = b0; b < b1; b++) {
        const int64_t bucket_start = integral_bucket_start(origin, width, b);
        uint32_t ka = 0, kb = 0;
        const uint64_t rows = change_regular_rows(start, delta, n, bucket_start, change_bucket_last(bucket_start, width), &ka, &kb);
        if (rows == 0) continue;
        CHECK(ka >= 1 && kb < n && rows == (uint64_t)(kb - ka) + 1);
        for (uint32_t k = ka; k <= kb; k++) closed[{b, key_at(k - 1), key_at(k)}] += 1;
    }
    if (closed != expected) {
        std::printf("MISMATCH %s: the row ranges give %zu counters, the reference %zu\n", name, closed.size(), expected.size());
        failures++;
    }
}

int main() {
    const int64_t none = INT64_MAX;
    auto level = [](int32_t key) { return [key](uint32_t) { return key; }; };
    auto saw = [](uint32_t k) { return (int32_t)((k * 7u) % 13u) - 3; };
    auto ramp = [](uint32_t k) { return (int32_t)k * 5 - 40; };
    // buckets that hold many rows, one row, no row; that begin behind the first row and end before the last; a bucket
    // edge on a row; a bucket inside one interval; one bucket over everything; a window of the buckets
    check_run("level", 1000, 100, 50, level(7), 0, 700, 0, 10, none);
    check_run("level clipped", 1000, 100, 50, level(-2), 1030, 333, 0, 20, none);
    check_run("ramp narrow", 1000, 100, 9, ramp, 990, 30, 0, 40, none);
    check_run("ramp edge on rows", 1000, 100, 50, ramp, 1000, 100, 0, 52, none);
    check_run("ramp two rows a bucket", 1000, 100, 50, ramp, 1000, 200, 0, 30, none);
    check_run("saw one bucket", 1000, 100, 50, saw, -5000, 100000, 0, 1, none);
    check_run("saw window", 1000, 100, 50, saw, 0, 450, 3, 9, none);
    check_run("saw unaligned", 1000, 100, 200, saw, 30, 333, 5, 31, none);
    check_run("one row", 500, 100, 1, level(1), 0, 300, 0, 4, none);
    check_run("two rows", 500, 100, 2, ramp, 0, 30, 10, 25, none);
    check_run("delta 1", -20, 1, 60, saw, -25, 7, 0, 12, none);
    // the gap rule: delta == max_gap links, delta > max_gap links nothing, max_gap 0 links nothing
    check_run("gap equal", 1000, 100, 20, saw, 0, 700, 0, 5, 100);
    check_run("gap exceeded", 1000, 100, 20, saw, 0, 700, 0, 5, 99);
    check_run("gap zero", 1000, 100, 20, saw, 0, 700, 0, 5, 0);
    // epoch-scale timestamps (microseconds)
    const int64_t epoch = 1658671178037000;
    check_run("epoch level", epoch, 1000000, 600, level(21), epoch - 12345, 7777777, 0, 80, none);
    check_run("epoch saw", epoch, 1000000, 600, saw, epoch - 12345, 60000000, 0, 12, none);
    // origin, width and timestamps at the int64 extremes: the far bucket requests (origin INT64_MIN, width INT64_MAX:
    // three buckets cover the axis, the last one row wide), a bucket whose last instant saturates, rows at INT64_MIN
    check_run("whole axis", -4000000000000000000, 2000000000000000000, 5, ramp, INT64_MIN, INT64_MAX, 0, 3, none);
    check_run("whole axis, first bucket", -4000000000000000000, 2000000000000000000, 5, ramp, INT64_MIN, INT64_MAX, 0, 1, none);
    check_run("saturating end", INT64_MAX - 1000, 100, 11, saw, INT64_MAX - 1050, 400, 0, 3, none);
    check_run("low origin", INT64_MIN, 4611686018427387904, 4, saw, INT64_MIN, 4611686018427387904, 0, 4, none);
    check_run("low origin, narrow", INT64_MIN + 5, 10, 8, ramp, INT64_MIN, 7, 0, 12, none);
    {
        // a step back in time links nothing and may land in an earlier bucket; equal timestamps link nothing; a pair
        // whose earlier row lies in front of the window counts, one whose later row lies behind it does not
        const std::vector<Point> points = {{500, 1}, {600, 2}, {100, 5}, {200, 7}, {200, 9}, {300, 1}, {900, 4}};
        const Pairs pairs = walk_pairs(points, none, 150, 250, 0, 2);
        CHECK(pairs == reference_pairs(points, none, 150, 250, 0, 2));
        // bucket 0 is [150, 400): 100 -> 200 (5 -> 7) and 200 -> 300 (9 -> 1); bucket 1 is [400, 650): 500 -> 600
        CHECK(pairs.size() == 3 && pairs.at({0, 5, 7}) == 1 && pairs.at({0, 9, 1}) == 1 && pairs.at({1, 1, 2}) == 1);
        const std::vector<Point> wide = {{-1000, 3}, {45, 4}, {100000, 5}};
        const Pairs through = walk_pairs(wide, none, 0, 10, 2, 7);
        CHECK(through.size() == 1 && through.at({4, 3, 4}) == 1);
        // the walk steps to the next bucket, jumps over empty ones and comes back
        const std::vector<Point> hops = {{0, 0}, {5, 1}, {12, 2}, {19, 3}, {20, 4}, {75, 5}, {76, 6}, {3, 7}, {4, 8}};
        const Pairs hopped = walk_pairs(hops, none, 0, 10, 0, 8);
        CHECK(hopped == reference_pairs(hops, none, 0, 10, 0, 8) && hopped.size() == 7);
        // gaps of 2^63 - 1 (the largest any max_gap links) and of 2^63 (never linked); the far request's buckets
        const std::vector<Point> far = {{INT64_MIN, 1}, {-1, 4}, {0, 6}, {INT64_MAX - 1, 2}, {INT64_MAX, 3}};
        const Pairs pairs2 = walk_pairs(far, none, INT64_MIN, INT64_MAX, 0, 3);
        CHECK(pairs2 == reference_pairs(far, none, INT64_MIN, INT64_MAX, 0, 3));
        // (bucket 0 ends at -2, bucket 1 is [-1, INT64_MAX - 2], bucket 2 holds the last two instants)
        CHECK(pairs2.size() == 4 && pairs2.at({1, 1, 4}) == 1 && pairs2.at({1, 4, 6}) == 1 && pairs2.at({2, 6, 2}) == 1 &&
              pairs2.at({2, 2, 3}) == 1);
        const Pairs gapped = walk_pairs(far, INT64_MAX - 1, INT64_MIN, INT64_MAX, 0, 3);
        CHECK(gapped == reference_pairs(far, INT64_MAX - 1, INT64_MIN, INT64_MAX, 0, 3));
        CHECK(gapped.size() == 3 && gapped.count({1, 1, 4}) == 0);
        CHECK(walk_pairs(far, none, INT64_MIN, INT64_MAX, 0, 1).empty());
        const std::vector<Point> ends = {{INT64_MIN, 1}, {INT64_MAX, 2}};
        CHECK(walk_pairs(ends, none, INT64_MIN, INT64_MAX, 0, 3).empty()); // (2^64 - 1 apart: beyond any max_gap)
    }

    // merge and crossings
    {
        uint64_t into[4] = {0, 5, UINT64_MAX - 1, 7}, from[4] = {3, 0, 3, 7};
        CHECK(mdb_transit_merge_n(into, from, 4) == 0);
        CHECK(into[0] == 3 && into[1] == 5 && into[2] == 1 && into[3] == 14); // (wraps, as uint64_t sums do)
        CHECK(mdb_transit_merge_n(nullptr, from, 1) == 1 && mdb_transit_merge_n(nullptr, nullptr, 0) == 0);
        // two rows of 3 x 3: [from][to]
        const uint64_t counts[18] = {1, 2, 3, 4, 5, 6, 7, 8, 9, /**/ 0, 0, 1, 0, 0, 0, 0, 0, 0};
        uint64_t up[4], down[4];
        CHECK(mdb_transit_crossings(counts, 2, 3, up, down) == 0);
        // edge 0: up 0 -> 1, 0 -> 2 = 2 + 3; down 1 -> 0, 2 -> 0 = 4 + 7. edge 1: up 0 -> 2, 1 -> 2 = 3 + 6; down 2 -> 0,
        // 2 -> 1 = 7 + 8
        CHECK(up[0] == 5 && down[0] == 11 && up[1] == 9 && down[1] == 15);
        CHECK(up[2] == 1 && up[3] == 1 && down[2] == 0 && down[3] == 0); // (a jump over two edges crosses both)
        // against the definition, on a 6 x 6 matrix
        uint64_t big[36], ups[5], downs[5];
        for (uint32_t k = 0; k < 36; k++) big[k] = (k * 2654435761u) % 97u;
        CHECK(mdb_transit_crossings(big, 1, 6, ups, downs) == 0);
        for (uint32_t e = 0; e < 5; e++) {
            uint64_t u = 0, d = 0;
            for (uint32_t a = 0; a < 6; a++)
                for (uint32_t b = 0; b < 6; b++) {
                    if (a <= e && e < b) u += big[a * 6 + b];
                    if (b <= e && e < a) d += big[a * 6 + b];
                }
            CHECK(ups[e] == u && downs[e] == d);
        }
        uint64_t one = 9;
        CHECK(mdb_transit_crossings(&one, 1, 1, nullptr, nullptr) == 0); // (one cell: no edge, nothing written)
        CHECK(mdb_transit_crossings(counts, 2, 0, up, down) == 1);
        CHECK(mdb_transit_crossings(counts, 2, 3, nullptr, down) == 1 && mdb_transit_crossings(nullptr, 1, 3, up, down) == 1);
        CHECK(mdb_transit_crossings(nullptr, 0, 3, nullptr, nullptr) == 0);
    }

    // malformed requests and edge lists fail before the device step and leave the counters alone
    {
        mdb_ctx *ctx = reinterpret_cast<mdb_ctx *>(8); // (never dereferenced)
        mdb_segments batch;
        std::memset(&batch, 0, sizeof(batch));
        batch.n = 3;
        const mdb_segments *inputs[1] = {&batch};
        const float edges[2] = {0.0f, 1.0f};
        uint64_t counts[36], before[36];
        std::memset(counts, 0xA5, sizeof(counts));
        std::memcpy(before, counts, sizeof(counts));
        const mdb_transit_request good = {{0, 100, 4, INT64_MIN, INT64_MAX, 1, 0}, INT64_MAX, 0, 0};
        struct Bad {
            mdb_transit_request request;
            const char *message;
        };
        std::vector<Bad> bad;
        auto with = [&](auto change, const char *message) {
            mdb_transit_request request = good;
            change(request);
            bad.push_back(Bad{request, message});
        };
        with([](mdb_transit_request &q) { q.buckets.which_mask = 1; }, "which_mask");
        with([](mdb_transit_request &q) { q.buckets.width = 0; }, "width");
        with([](mdb_transit_request &q) { q.buckets.width = -7; }, "width");
        with([](mdb_transit_request &q) { q.buckets.n_groups = 0; }, "n_groups must");
        with([](mdb_transit_request &q) { q.buckets.n_groups = 4000000000u; q.buckets.n_buckets = 1ull << 60; }, "overflows");
        with([](mdb_transit_request &q) { q.buckets.n_buckets = 1ull << 57; }, "overflows"); // (2^57 * 9 > 2^60)
        with([](mdb_transit_request &q) { q.buckets.t_lo = 0; }, "time range");
        with([](mdb_transit_request &q) { q.buckets.t_hi = 1000; }, "time range");
        with([](mdb_transit_request &q) { q.reserved = 1; }, "reserved");
        with([](mdb_transit_request &q) { q.flags = 1; }, "flags");
        with([](mdb_transit_request &q) { q.max_gap = -1; }, "max_gap");
        for (const Bad &b : bad) {
            CHECK(mdb_transit_buckets(ctx, &batch, nullptr, &b.request, edges, 2, counts) == 1);
            CHECK(g_last_error.find(b.message) != std::string::npos);
            CHECK(mdb_transit_buckets_list(ctx, inputs, nullptr, 1, &b.request, edges, 2, counts) == 1);
            CHECK(g_last_error.find(b.message) != std::string::npos);
        }
        // the square of the cells counts: 2^36 rows fit under 2 edges and not under 4 095
        {
            mdb_transit_request request = good;
            request.buckets.n_buckets = 1ull << 36;
            uint64_t n_rows = 0;
            CHECK(transit_request_check(&request, 2, &n_rows) == 0 && n_rows == 1ull << 36);
            CHECK(transit_request_check(&request, MDB_HIST_MAX_EDGES, &n_rows) == 1);
        }
        const float descending[2] = {1.0f, 0.0f}, twice[2] = {1.0f, 1.0f}, zeros[2] = {0.0f, -0.0f};
        for (const float *wrong : {descending, twice, zeros}) {
            CHECK(mdb_transit_buckets(ctx, &batch, nullptr, &good, wrong, 2, counts) == 1);
            CHECK(g_last_error.find("strictly increasing") != std::string::npos);
        }
        CHECK(mdb_transit_buckets(ctx, &batch, nullptr, &good, edges, 0, counts) == 1 && g_last_error.find("n_edges") != std::string::npos);
        CHECK(mdb_transit_buckets(ctx, &batch, nullptr, &good, edges, MDB_HIST_MAX_EDGES + 1, counts) == 1);
        CHECK(mdb_transit_buckets(nullptr, &batch, nullptr, &good, edges, 2, counts) == 1);
        CHECK(mdb_transit_buckets(ctx, nullptr, nullptr, &good, edges, 2, counts) == 1);
        CHECK(mdb_transit_buckets(ctx, &batch, nullptr, nullptr, edges, 2, counts) == 1);
        CHECK(mdb_transit_buckets(ctx, &batch, nullptr, &good, nullptr, 2, counts) == 1);
        CHECK(mdb_transit_buckets(ctx, &batch, nullptr, &good, edges, 2, nullptr) == 1);
        const mdb_segments *missing[1] = {nullptr};
        CHECK(mdb_transit_buckets_list(ctx, missing, nullptr, 1, &good, edges, 2, counts) == 1);
        CHECK(device_calls == 0);
        CHECK(std::memcmp(counts, before, sizeof(counts)) == 0);
        // nothing to do: success without the device
        mdb_transit_request no_buckets = good;
        no_buckets.buckets.n_buckets = 0;
        CHECK(mdb_transit_buckets(ctx, &batch, nullptr, &no_buckets, edges, 2, counts) == 0);
        CHECK(mdb_transit_buckets_list(ctx, inputs, nullptr, 0, &good, edges, 2, counts) == 0);
        CHECK(device_calls == 0);
        CHECK(mdb_transit_buckets(ctx, &batch, nullptr, &good, edges, 2, counts) == 0);
        CHECK(device_calls == 1);
        CHECK(std::memcmp(counts, before, sizeof(counts)) == 0);
    }

    if (failures) {
        std::printf("%d MISMATCH(es)\n", failures);
        return 1;
    }
    std::printf("ok: pair walks, row ranges on regular timestamps, merge, crossings, request and edge checks\n");
    return 0;
}
