// check_dwell_host.cpp - TEST INFRASTRUCTURE: the part of the dwell operator that needs no GPU. The bucket walk of one
// linked interval (dwell_interval), the walk of a run of rows (dwell_walk_point) and the pieces of one bucket among
// rows on regular timestamps (dwell_regular_bucket) of mdb_dwell.hpp are compared with an interval-by-interval
// evaluation in 128-bit integers; mdb_dwell_merge_n and mdb_dwell_share are checked on counters; and the host forms
// (mdb_dwell_host.cpp) are handed malformed requests and edge lists: they must fail with their messages before
// dwell_list_run - here a stand-in that counts its calls - is reached, and leave the counters alone.
#include "../../modelardb-rs_amd/csrc/mdb_dwell.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int dwell_list_run(mdb_ctx *, const mdb_segments *const *, const uint32_t *const *, uint32_t, const mdb_dwell_request *,
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

using Cells = std::map<std::pair<uint64_t, int32_t>, uint64_t>; // (bucket, key) -> microseconds

// Interval by interval, bucket [start, end) as 128-bit integers (nothing wraps or saturates here).
static Cells reference_cells(const std::vector<Point> &points, int64_t max_gap, int64_t origin, int64_t width, uint64_t b0,
                             uint64_t b1) {
    Cells cells;
    for (size_t k = 0; k + 1 < points.size(); k++) {
        const __int128 t0 = points[k].t, t1 = points[k + 1].t;
        if (t1 <= t0 || t1 - t0 > (__int128)max_gap) continue;
        for (uint64_t b = b0; b < b1; b++) {
            const __int128 start = (__int128)origin + (__int128)b * width, end = start + width;
            const __int128 a = t0 > start ? t0 : start, e = t1 < end ? t1 : end;
            if (e > a) cells[{b, points[k].key}] += (uint64_t)(e - a);
        }
    }
    return cells;
}

static Cells walk_cells(const std::vector<Point> &points, int64_t max_gap, int64_t origin, int64_t width, uint64_t b0,
                        uint64_t b1) {
    Cells cells;
    const DwellWindow w = {origin, width, max_gap, b0, b1};
    DwellWalk walk = dwell_walk_start();
    for (const Point &p : points)
        dwell_walk_point(w, walk, p.t, p.key, [&](uint64_t b, int32_t key, uint64_t length) {
            CHECK(b >= b0 && b < b1 && length > 0);
            cells[{b, key}] += length;
        });
    return cells;
}

// A run of n rows start + k * delta with keys key_at(k): the walk against the reference in every bucket of [b0, b1),
// and, where the gap rule links the rows, dwell_regular_bucket's pieces against both.
template <typename KeyAt>
static void check_run(const char *name, int64_t start, int64_t delta, uint32_t n, KeyAt key_at, int64_t origin, int64_t width,
                      uint64_t b0, uint64_t b1, int64_t max_gap) {
    std::vector<Point> points;
    for (uint32_t k = 0; k < n; k++) points.push_back(Point{(int64_t)((uint64_t)start + (uint64_t)k * (uint64_t)delta), key_at(k)});
    const Cells expected = reference_cells(points, max_gap, origin, width, b0, b1);
    const Cells walked = walk_cells(points, max_gap, origin, width, b0, b1);
    if (walked != expected) {
        std::printf("MISMATCH %s: the walk gives %zu cells, the reference %zu\n", name, walked.size(), expected.size());
        failures++;
    }
    if (!integral_linked(max_gap, 0, delta)) {
        CHECK(expected.empty());
        return;
    }
    Cells closed;
    for (uint64_t b = b0; b < b1; b++) {
        const int64_t bucket_start = integral_bucket_start(origin, width, b);
        const DwellRegular p = dwell_regular_bucket(start, delta, n, bucket_start, integral_bucket_end(bucket_start, width));
        if (p.head) closed[{b, key_at(p.head_row)}] += p.head;
        for (uint32_t k = p.ka; k < p.kb; k++) closed[{b, key_at(k)}] += (uint64_t)delta;
        if (p.tail) closed[{b, key_at(p.kb)}] += p.tail;
        if (p.head) CHECK(p.head_row + 1 < n && p.head <= (uint64_t)delta);
        if (p.tail) CHECK(p.kb + 1 < n && p.tail < (uint64_t)delta);
        CHECK(p.kb < n && p.ka <= p.kb + 1);
    }
    if (closed != expected) {
        std::printf("MISMATCH %s: the pieces give %zu cells, the reference %zu\n", name, closed.size(), expected.size());
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
    // origin, width and timestamps at the int64 extremes: one bucket over everything, a bucket whose end saturates,
    // rows at INT64_MIN
    check_run("whole axis", -4000000000000000000, 2000000000000000000, 5, ramp, INT64_MIN, INT64_MAX, 0, 2, none);
    check_run("saturating end", INT64_MAX - 1000, 100, 11, saw, INT64_MAX - 1050, 400, 0, 3, none);
    check_run("low origin", INT64_MIN, 4611686018427387904, 4, saw, INT64_MIN, 4611686018427387904, 0, 4, none);
    check_run("low origin, narrow", INT64_MIN + 5, 10, 8, ramp, INT64_MIN, 7, 0, 12, none);
    {
        // a step back in time links nothing and may land in an earlier bucket; equal timestamps link nothing; the
        // last row holds nothing; an interval whose ends lie outside every bucket still fills the buckets between
        const std::vector<Point> points = {{500, 1}, {600, 2}, {100, 5}, {200, 7}, {200, 9}, {300, 1}, {900, 4}};
        const Cells cells = walk_cells(points, none, 150, 250, 0, 2);
        CHECK(cells == reference_cells(points, none, 150, 250, 0, 2));
        CHECK(cells.at({0, 5}) == 50 && cells.at({0, 9}) == 100 && cells.at({0, 1}) == 100 && cells.at({1, 1}) == 350);
        CHECK(cells.size() == 4);
        const std::vector<Point> wide = {{-1000, 3}, {100000, 4}};
        const Cells through = walk_cells(wide, none, 0, 10, 2, 7);
        CHECK(through.size() == 5);
        for (uint64_t b = 2; b < 7; b++) CHECK(through.at({b, 3}) == 10);
        // gaps of 2^63 - 1 (the largest any max_gap links) and of 2^63 (never linked)
        const std::vector<Point> far = {{INT64_MIN, 1}, {-1, 4}, {INT64_MAX, 2}};
        Cells cells2 = walk_cells(far, none, INT64_MIN, INT64_MAX, 0, 3);
        CHECK(cells2 == reference_cells(far, none, INT64_MIN, INT64_MAX, 0, 3));
        CHECK(cells2.size() == 1 && cells2.at({0, 1}) == (uint64_t)INT64_MAX);
        CHECK(walk_cells(far, INT64_MAX - 1, INT64_MIN, INT64_MAX, 0, 3).empty());
    }

    // merge and share
    {
        uint64_t into[4] = {0, 5, UINT64_MAX - 1, 7}, from[4] = {3, 0, 3, 7};
        CHECK(mdb_dwell_merge_n(into, from, 4) == 0);
        CHECK(into[0] == 3 && into[1] == 5 && into[2] == 1 && into[3] == 14); // (wraps, as uint64_t sums do)
        CHECK(mdb_dwell_merge_n(nullptr, from, 1) == 1 && mdb_dwell_merge_n(nullptr, nullptr, 0) == 0);
        const uint64_t dwell[9] = {1, 1, 2, 0, 0, 0, UINT64_MAX, UINT64_MAX, 0};
        double out[9];
        CHECK(mdb_dwell_share(dwell, 3, 3, out) == 0);
        CHECK(out[0] == 0.25 && out[1] == 0.25 && out[2] == 0.5);
        CHECK(std::isnan(out[3]) && std::isnan(out[4]) && std::isnan(out[5]));
        CHECK(out[6] == 0.5 && out[7] == 0.5 && out[8] == 0.0); // (the row's total is formed beyond 64 bits)
        CHECK(mdb_dwell_share(dwell, 1, 3, nullptr) == 1 && mdb_dwell_share(nullptr, 0, 3, nullptr) == 0);
    }

    // malformed requests and edge lists fail before the device step and leave the counters alone
    {
        mdb_ctx *ctx = reinterpret_cast<mdb_ctx *>(8); // (never dereferenced)
        mdb_segments batch;
        std::memset(&batch, 0, sizeof(batch));
        batch.n = 3;
        const mdb_segments *inputs[1] = {&batch};
        const float edges[2] = {0.0f, 1.0f};
        uint64_t dwell[12], before[12];
        std::memset(dwell, 0xA5, sizeof(dwell));
        std::memcpy(before, dwell, sizeof(dwell));
        const mdb_dwell_request good = {{0, 100, 4, INT64_MIN, INT64_MAX, 1, 0}, INT64_MAX, MDB_DWELL_STEP, 0};
        struct Bad {
            mdb_dwell_request request;
            const char *message;
        };
        std::vector<Bad> bad;
        auto with = [&](auto change, const char *message) {
            mdb_dwell_request request = good;
            change(request);
            bad.push_back(Bad{request, message});
        };
        with([](mdb_dwell_request &q) { q.buckets.which_mask = 1; }, "which_mask");
        with([](mdb_dwell_request &q) { q.buckets.width = 0; }, "width");
        with([](mdb_dwell_request &q) { q.buckets.width = -7; }, "width");
        with([](mdb_dwell_request &q) { q.buckets.n_groups = 0; }, "n_groups must");
        with([](mdb_dwell_request &q) { q.buckets.n_groups = 4000000000u; q.buckets.n_buckets = 1ull << 60; }, "overflows");
        with([](mdb_dwell_request &q) { q.buckets.n_buckets = 1ull << 59; }, "overflows");
        with([](mdb_dwell_request &q) { q.buckets.t_lo = 0; }, "time range");
        with([](mdb_dwell_request &q) { q.buckets.t_hi = 1000; }, "time range");
        with([](mdb_dwell_request &q) { q.method = MDB_INTEGRAL_LINEAR; }, "MDB_INTEGRAL_LINEAR");
        with([](mdb_dwell_request &q) { q.method = 2; }, "Unknown method");
        with([](mdb_dwell_request &q) { q.flags = 1; }, "flags");
        with([](mdb_dwell_request &q) { q.max_gap = -1; }, "max_gap");
        for (const Bad &b : bad) {
            CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, &b.request, edges, 2, dwell) == 1);
            CHECK(g_last_error.find(b.message) != std::string::npos);
            CHECK(mdb_dwell_buckets_list(ctx, inputs, nullptr, 1, &b.request, edges, 2, dwell) == 1);
            CHECK(g_last_error.find(b.message) != std::string::npos);
        }
        const float descending[2] = {1.0f, 0.0f}, twice[2] = {1.0f, 1.0f}, zeros[2] = {0.0f, -0.0f};
        for (const float *wrong : {descending, twice, zeros}) {
            CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, &good, wrong, 2, dwell) == 1);
            CHECK(g_last_error.find("strictly increasing") != std::string::npos);
        }
        CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, &good, edges, 0, dwell) == 1 && g_last_error.find("n_edges") != std::string::npos);
        CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, &good, edges, MDB_HIST_MAX_EDGES + 1, dwell) == 1);
        CHECK(mdb_dwell_buckets(nullptr, &batch, nullptr, &good, edges, 2, dwell) == 1);
        CHECK(mdb_dwell_buckets(ctx, nullptr, nullptr, &good, edges, 2, dwell) == 1);
        CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, nullptr, edges, 2, dwell) == 1);
        CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, &good, nullptr, 2, dwell) == 1);
        CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, &good, edges, 2, nullptr) == 1);
        const mdb_segments *missing[1] = {nullptr};
        CHECK(mdb_dwell_buckets_list(ctx, missing, nullptr, 1, &good, edges, 2, dwell) == 1);
        CHECK(device_calls == 0);
        CHECK(std::memcmp(dwell, before, sizeof(dwell)) == 0);
        // nothing to do: success without the device
        mdb_dwell_request no_buckets = good;
        no_buckets.buckets.n_buckets = 0;
        CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, &no_buckets, edges, 2, dwell) == 0);
        CHECK(mdb_dwell_buckets_list(ctx, inputs, nullptr, 0, &good, edges, 2, dwell) == 0);
        CHECK(device_calls == 0);
        CHECK(mdb_dwell_buckets(ctx, &batch, nullptr, &good, edges, 2, dwell) == 0);
        CHECK(device_calls == 1);
        CHECK(std::memcmp(dwell, before, sizeof(dwell)) == 0);
    }

    if (failures) {
        std::printf("%d MISMATCH(es)\n", failures);
        return 1;
    }
    std::printf("ok: interval walks, pieces on regular timestamps, merge, share, request and edge checks\n");
    return 0;
}
