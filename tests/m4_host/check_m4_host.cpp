// check_m4_host.cpp - TEST INFRASTRUCTURE: the entry points of M4 downsampling that run before the device is needed
// (mdb_m4_host.cpp), without a GPU. mdb_m4_merge_n is compared with a restatement of the four rules on sorted points,
// and the host forms are handed malformed requests: they must fail with their messages before m4_list_run - here a
// stand-in that counts its calls - is reached, and leave the cells alone.
#include "../../modelardb-rs_amd/csrc/mdb_m4.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <random>
#include <tuple>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int m4_list_run(mdb_ctx *, const mdb_segments *const *, const uint32_t *const *, uint32_t, const mdb_bucket_request *,
                uint64_t, mdb_m4_cell *) {
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

static float from_bits(uint32_t bits) {
    float v;
    std::memcpy(&v, &bits, 4);
    return v;
}

struct Point {
    int64_t t;
    float v;
};

// The four rules restated: sort the points, take the ends.
static mdb_m4_cell cell_of(std::vector<Point> points) {
    mdb_m4_cell cell;
    std::memset(&cell, 0, sizeof cell);
    if (points.empty()) return cell;
    auto by_time = [](const Point &a, const Point &b) { return std::make_tuple(a.t, m4_key(a.v)) < std::make_tuple(b.t, m4_key(b.v)); };
    auto by_low = [](const Point &a, const Point &b) { return std::make_tuple(m4_key(a.v), a.t) < std::make_tuple(m4_key(b.v), b.t); };
    auto by_high = [](const Point &a, const Point &b) { return std::make_tuple(-(int64_t)m4_key(a.v), a.t) < std::make_tuple(-(int64_t)m4_key(b.v), b.t); };
    cell.count = (int64_t)points.size();
    const Point first = *std::min_element(points.begin(), points.end(), by_time);
    const Point last = *std::max_element(points.begin(), points.end(), by_time);
    const Point low = *std::min_element(points.begin(), points.end(), by_low);
    const Point high = *std::min_element(points.begin(), points.end(), by_high);
    cell.t_first = first.t, cell.v_first = first.v, cell.t_last = last.t, cell.v_last = last.v;
    cell.t_min = low.t, cell.v_min = low.v, cell.t_max = high.t, cell.v_max = high.v;
    return cell;
}

int main() {
    const uint32_t specials[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7fc00001u,
                                 0x3f800000u, 0xbf800000u, 0x00000001u, 0x80000001u, 0x7f7fffffu, 0xff7fffffu};
    std::mt19937_64 rng(20261018);
    auto random_points = [&](size_t n) {
        std::vector<Point> points(n);
        for (Point &p : points) {
            p.t = rng() % 4 == 0 ? (int64_t)rng() : (int64_t)(rng() % 5) - 2;                 // (many equal timestamps)
            p.v = rng() % 3 == 0 ? from_bits((uint32_t)rng()) : from_bits(specials[rng() % 13]); // (many equal values)
        }
        return points;
    };
    // mdb_m4_merge_n: cells of random point sets merged pairwise = the cell of the union; commutative, associative
    for (int trial = 0; trial < 2000; trial++) {
        std::vector<Point> a = random_points(rng() % 5), b = random_points(rng() % 5), c = random_points(rng() % 3);
        std::vector<Point> ab = a, abc;
        ab.insert(ab.end(), b.begin(), b.end());
        abc = ab;
        abc.insert(abc.end(), c.begin(), c.end());
        mdb_m4_cell into[2] = {cell_of(a), cell_of(b)};
        const mdb_m4_cell from[2] = {cell_of(b), cell_of(a)}, expected = cell_of(ab);
        CHECK(mdb_m4_merge_n(into, from, 2) == 0);
        if (!ab.empty()) CHECK(std::memcmp(&into[0], &expected, sizeof expected) == 0 && std::memcmp(&into[1], &expected, sizeof expected) == 0);
        else CHECK(into[0].count == 0 && into[1].count == 0);
        mdb_m4_cell left = into[0], right = cell_of(b);
        const mdb_m4_cell third = cell_of(c), all = cell_of(abc);
        CHECK(mdb_m4_merge_n(&left, &third, 1) == 0);                                  // (a + b) + c
        CHECK(mdb_m4_merge_n(&right, &third, 1) == 0);                                 // a + (b + c)
        mdb_m4_cell grouped = cell_of(a);
        CHECK(mdb_m4_merge_n(&grouped, &right, 1) == 0);
        if (!abc.empty()) CHECK(std::memcmp(&left, &all, sizeof all) == 0 && std::memcmp(&grouped, &all, sizeof all) == 0);
    }
    // an empty `from` keeps every byte of `into`, also of an empty one; an empty `into` takes `from`
    mdb_m4_cell pattern, empty, some = cell_of(random_points(4));
    std::memset(&pattern, 0xA5, sizeof pattern);
    std::memset(&empty, 0, sizeof empty);
    pattern.count = 0;
    mdb_m4_cell kept = pattern;
    CHECK(mdb_m4_merge_n(&kept, &empty, 1) == 0 && std::memcmp(&kept, &pattern, sizeof pattern) == 0);
    CHECK(mdb_m4_merge_n(&kept, &some, 1) == 0 && std::memcmp(&kept, &some, sizeof some) == 0);
    CHECK(mdb_m4_merge_n(nullptr, nullptr, 0) == 0 && mdb_m4_merge_n(nullptr, &some, 1) == 1 && mdb_m4_merge_n(&kept, nullptr, 1) == 1);

    // the host forms: malformed requests fail before the device step, with the messages of mdb_agg_buckets
    mdb_ctx *fake_context = reinterpret_cast<mdb_ctx *>(8); // (never dereferenced)
    mdb_segments batch;
    std::memset(&batch, 0, sizeof batch);
    batch.n = 1;
    const mdb_segments *inputs[1] = {&batch};
    const mdb_segments *with_null[1] = {nullptr};
    mdb_m4_cell cells[4];
    std::memset(cells, 0xA5, sizeof cells);
    struct Bad {
        mdb_bucket_request request;
        const char *message;
    };
    const Bad bad[] = {{{0, 100, 4, INT64_MIN, INT64_MAX, 1, 1}, "which_mask must be 0 for mdb_m4_buckets*."},
                       {{0, 0, 4, INT64_MIN, INT64_MAX, 1, 0}, "The bucket width must be positive."},
                       {{0, -7, 4, INT64_MIN, INT64_MAX, 1, 0}, "The bucket width must be positive."},
                       {{0, 100, 4, INT64_MIN, INT64_MAX, 0, 0}, "n_groups must be at least 1."},
                       {{0, 100, UINT64_MAX / 8, INT64_MIN, INT64_MAX, 4000000000u, 0}, "n_groups * n_buckets overflows."}};
    for (const Bad &b : bad) {
        CHECK(mdb_m4_buckets_list(fake_context, inputs, nullptr, 1, &b.request, cells) == 1 && g_last_error == b.message);
        g_last_error.clear();
        CHECK(mdb_m4_buckets(fake_context, &batch, nullptr, &b.request, cells) == 1 && g_last_error == b.message);
    }
    const mdb_bucket_request good = {0, 100, 4, INT64_MIN, INT64_MAX, 1, 0}, no_buckets = {0, 100, 0, INT64_MIN, INT64_MAX, 1, 0};
    CHECK(mdb_m4_buckets_list(nullptr, inputs, nullptr, 1, &good, cells) == 1 && g_last_error.find("NULL") != std::string::npos);
    CHECK(mdb_m4_buckets_list(fake_context, nullptr, nullptr, 1, &good, cells) == 1);
    CHECK(mdb_m4_buckets_list(fake_context, inputs, nullptr, 1, nullptr, cells) == 1);
    CHECK(mdb_m4_buckets_list(fake_context, inputs, nullptr, 1, &good, nullptr) == 1);
    CHECK(mdb_m4_buckets(fake_context, nullptr, nullptr, &good, cells) == 1);
    CHECK(mdb_m4_buckets_list(fake_context, with_null, nullptr, 1, &good, cells) == 1 && g_last_error == "A batch of the list is NULL.");
    CHECK(device_calls == 0);
    // nothing to do: success without the device
    batch.n = 0;
    CHECK(mdb_m4_buckets_list(fake_context, inputs, nullptr, 1, &good, cells) == 0);
    CHECK(mdb_m4_buckets_list(fake_context, inputs, nullptr, 0, &good, cells) == 0);
    batch.n = 1;
    CHECK(mdb_m4_buckets_list(fake_context, inputs, nullptr, 1, &no_buckets, cells) == 0 && device_calls == 0);
    CHECK(mdb_m4_buckets_list(fake_context, inputs, nullptr, 1, &good, cells) == 0 && device_calls == 1);
    for (const mdb_m4_cell &cell : cells) {
        mdb_m4_cell untouched;
        std::memset(&untouched, 0xA5, sizeof untouched);
        CHECK(std::memcmp(&cell, &untouched, sizeof cell) == 0);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok: the host side of M4 downsampling\n");
    return 0;
}
