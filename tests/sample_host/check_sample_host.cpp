// check_sample_host.cpp - TEST INFRASTRUCTURE: the part of the sampling operator that needs no GPU. The instant
// arithmetic of mdb_sample.hpp (which instants a closed extent or an open interval contains, whether a timestamp lies
// on one) is compared with the same questions asked in 128-bit integers, at the int64 extremes: origin INT64_MIN,
// width INT64_MAX, timestamps next to both ends, t1 - t0 near 2^64. f(T) is compared with long double; the walk of a run
// of rows over a window of instants with a row-by-row evaluation; mdb_sample_merge_n and mdb_sample_values are checked
// on cells; and the host forms (mdb_sample_host.cpp) are handed malformed requests: they must fail with their messages
// before sample_list_run - here a stand-in that counts its calls - is reached, and leave the cells alone.
#include "../../modelardb-rs_amd/csrc/mdb_sample.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int sample_list_run(mdb_ctx *, const mdb_segments *const *, const uint32_t *const *, uint32_t, const mdb_sample_request *,
                    uint64_t, mdb_sample_cell *) {
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

typedef __int128 wide;

// The instants k < n with a <= origin + k * width <= e, in 128-bit integers: [first, first + count).
static unsigned __int128 reference_closed(wide origin, wide width, wide n, wide a, wide e, wide *first) {
    if (n == 0 || e < a || e < origin) return 0;
    wide k0 = a <= origin ? 0 : (a - origin + width - 1) / width;
    wide k1 = (e - origin) / width;
    if (k1 > n - 1) k1 = n - 1;
    if (k0 > k1) return 0;
    *first = k0;
    return (unsigned __int128)(k1 - k0 + 1);
}

static void check_instants(int64_t origin, int64_t width, uint64_t n, int64_t a, int64_t e) {
    uint64_t first = 0;
    wide expected_first = 0;
    const uint64_t count = sample_instants_closed(origin, width, n, a, e, &first);
    const unsigned __int128 expected = reference_closed(origin, width, (wide)n, a, e, &expected_first);
    if ((unsigned __int128)count != expected || (count && (wide)first != expected_first)) {
        std::printf("MISMATCH closed: origin %lld width %lld n %llu [%lld, %lld]: %llu from %llu\n", (long long)origin,
                    (long long)width, (unsigned long long)n, (long long)a, (long long)e, (unsigned long long)count,
                    (unsigned long long)first);
        failures++;
    }
    if (count) { // the instants formed are exact
        CHECK((wide)sample_instant(origin, width, first) == (wide)origin + (wide)first * width);
        CHECK((wide)sample_instant(origin, width, first + count - 1) == (wide)origin + (wide)(first + count - 1) * width);
        CHECK(sample_instant(origin, width, first) >= a && sample_instant(origin, width, first + count - 1) <= e);
    }
    if (e > a) { // the open interval (a, e)
        uint64_t open_first = 0;
        wide open_expected_first = 0;
        const uint64_t open = sample_instants_open(origin, width, n, a, e, &open_first);
        const unsigned __int128 open_expected = reference_closed(origin, width, (wide)n, (wide)a + 1, (wide)e - 1, &open_expected_first);
        CHECK((unsigned __int128)open == open_expected);
        if (open) CHECK((wide)open_first == open_expected_first);
    }
    for (int64_t t : {a, e}) { // a timestamp on an instant
        uint64_t k = 0;
        const bool on = sample_on_instant(origin, width, n, t, &k);
        const wide d = (wide)t - origin;
        const bool expected_on = d >= 0 && d % width == 0 && d / width < (wide)n;
        CHECK(on == expected_on);
        if (on && expected_on) CHECK((wide)k == d / width);
    }
}

struct Row {
    int64_t t;
    float v;
};

// Rows through the walk, over instants [k0, k1) of (origin, width): every row contributes.
static std::vector<mdb_sample_cell> walk_cells(const std::vector<Row> &rows, int64_t origin, int64_t width, uint64_t k0,
                                               uint64_t k1, int64_t max_gap, uint32_t method) {
    std::vector<mdb_sample_cell> cells(k1 - k0, mdb_sample_cell{0, 0.0});
    const SampleWindow w = sample_window(origin, width, max_gap, method, k0, k1, cells.data());
    SampleWalk walk = sample_walk_start();
    for (const Row &row : rows) sample_walk_point(w, walk, row.t, row.v, true);
    return cells;
}

// The same cells row by row and interval by interval, in 128-bit integers and long double.
static void check_walk(const char *name, const std::vector<Row> &rows, int64_t origin, int64_t width, uint64_t k0,
                       uint64_t k1, int64_t max_gap, uint32_t method) {
    const std::vector<mdb_sample_cell> cells = walk_cells(rows, origin, width, k0, k1, max_gap, method);
    for (uint64_t k = k0; k < k1; k++) {
        const wide at = (wide)origin + (wide)k * width;
        uint64_t count = 0;
        long double sum = 0.0L, scale = 0.0L;
        for (size_t r = 0; r < rows.size(); r++) {
            if ((wide)rows[r].t == at) {
                count++;
                sum += rows[r].v;
                scale += std::fabs(rows[r].v);
            }
            if (method == MDB_SAMPLE_EXACT || r + 1 == rows.size()) continue;
            const wide t0 = rows[r].t, t1 = rows[r + 1].t;
            if (t1 <= t0 || t1 - t0 > (wide)max_gap || !(t0 < at && at < t1)) continue;
            const long double v0 = rows[r].v, v1 = rows[r + 1].v;
            count++;
            sum += method == MDB_SAMPLE_STEP ? v0 : v0 + (v1 - v0) * ((long double)(at - t0) / (long double)(t1 - t0));
            scale += std::fmax(std::fabs(v0), std::fabs(v1));
        }
        const mdb_sample_cell &cell = cells[k - k0];
        // (2^-48 of the scale is the contract; long double carries 2^-64)
        if (cell.count != count || !(std::fabs((long double)cell.sum - sum) <= 0x1p-48L * scale)) {
            std::printf("MISMATCH walk %s: instant %llu: count %llu (expected %llu), sum %.17g (expected %.17Lg)\n", name,
                        (unsigned long long)k, (unsigned long long)cell.count, (unsigned long long)count, cell.sum, sum);
            failures++;
        }
    }
}

int main() {
    // the instants of extents and intervals at the int64 extremes
    {
        const int64_t origins[] = {INT64_MIN, INT64_MIN + 1, -1000, 0, 7, INT64_MAX - 1000, INT64_MAX};
        const int64_t widths[] = {1, 2, 3, 100, 1000, INT64_MAX / 2, INT64_MAX - 1, INT64_MAX};
        const uint64_t counts[] = {0, 1, 2, 3, 1000, UINT64_MAX / 2, UINT64_MAX};
        const int64_t times[] = {INT64_MIN, INT64_MIN + 1, INT64_MIN + 2, -1001, -1000, -999, -1, 0, 1, 6, 7, 8, 99, 100, 101,
                                 INT64_MAX / 2, INT64_MAX - 1001, INT64_MAX - 1000, INT64_MAX - 2, INT64_MAX - 1, INT64_MAX};
        for (int64_t origin : origins)
            for (int64_t width : widths)
                for (uint64_t n : counts)
                    for (int64_t a : times)
                        for (int64_t e : times) check_instants(origin, width, n, a, e);
        // t1 - t0 == 2^64 - 1, origin INT64_MIN, width INT64_MAX: instants INT64_MIN, -1 and INT64_MAX - 1
        uint64_t first = 99;
        CHECK(sample_instants_closed(INT64_MIN, INT64_MAX, UINT64_MAX, INT64_MIN, INT64_MAX, &first) == 3 && first == 0);
        CHECK(sample_instant(INT64_MIN, INT64_MAX, 1) == -1 && sample_instant(INT64_MIN, INT64_MAX, 2) == INT64_MAX - 1);
        CHECK(sample_instants_open(INT64_MIN, INT64_MAX, UINT64_MAX, INT64_MIN, INT64_MAX, &first) == 2 && first == 1);
        CHECK(sample_instants_open(INT64_MIN, 1, UINT64_MAX, INT64_MIN, INT64_MAX, &first) == UINT64_MAX - 1 && first == 1);
        CHECK(sample_instants_open(0, 1, 10, 4, 5, &first) == 0 && sample_instants_open(0, 1, 10, 5, 4, &first) == 0);
        CHECK(sample_linked(INT64_MAX, INT64_MIN, INT64_MAX) == false); // (the gap is 2^64 - 1)
        CHECK(sample_linked(INT64_MAX, -1, INT64_MAX - 1) && !sample_linked(INT64_MAX, -2, INT64_MAX - 1));
        CHECK(!sample_linked(0, 5, 6) && !sample_linked(100, 5, 5) && !sample_linked(100, 6, 5) && sample_linked(1, 5, 6));
    }

    // f(T) against long double, time differences near 2^64 included
    {
        const float values[] = {0.0f, -0.0f, 1.0f, -3.5f, 1.0e-30f, 3.0e38f, -3.0e38f, 123.456f};
        const int64_t spans[][3] = {{0, 100, 37}, {-50, 50, -49}, {INT64_MIN, INT64_MAX, -1}, {INT64_MIN, INT64_MAX, INT64_MAX - 1},
                                    {INT64_MIN, INT64_MAX, INT64_MIN + 1}, {INT64_MAX - 2, INT64_MAX, INT64_MAX - 1},
                                    {1658671178037000, 1658671178137000, 1658671178100001}};
        for (const auto &span : spans)
            for (float v0 : values)
                for (float v1 : values) {
                    const int64_t t0 = span[0], t1 = span[1], at = span[2];
                    const long double part = (long double)((wide)at - t0) / (long double)((wide)t1 - t0);
                    const long double linear = (long double)v0 + ((long double)v1 - (long double)v0) * part;
                    const long double scale = std::fmax(std::fabs(v0), std::fabs(v1));
                    const double got = sample_value(MDB_SAMPLE_LINEAR, t0, v0, t1, v1, at);
                    CHECK(std::fabs((long double)got - linear) <= 0x1p-50L * scale);
                    if (v0 == v1) CHECK(got == (double)v0);
                    CHECK(sample_value(MDB_SAMPLE_STEP, t0, v0, t1, v1, at) == (double)v0);
                }
        CHECK(std::isnan(sample_value(MDB_SAMPLE_LINEAR, 0, NAN, 10, 1.0f, 5)));
        CHECK(std::isnan(sample_value(MDB_SAMPLE_LINEAR, 0, 1.0f, 10, NAN, 5)));
        CHECK(!std::isfinite(sample_value(MDB_SAMPLE_LINEAR, 0, 1.0f, 10, INFINITY, 5)));
        CHECK(!std::isfinite(sample_value(MDB_SAMPLE_LINEAR, 0, INFINITY, 10, -INFINITY, 5)));
        CHECK(sample_value(MDB_SAMPLE_LINEAR, 0, INFINITY, 10, INFINITY, 5) == INFINITY);
        CHECK(sample_value(MDB_SAMPLE_STEP, 0, 1.0f, 10, NAN, 5) == 1.0);
    }

    // the cell add: the first contribution is taken whole
    {
        mdb_sample_cell cell = {0, 0.0};
        sample_cell_contribute(cell, -0.0);
        CHECK(cell.count == 1 && std::signbit(cell.sum));
        sample_cell_contribute(cell, 2.5);
        CHECK(cell.count == 2 && cell.sum == 2.5);
        mdb_sample_cell other = {0, 123.0}; // (count 0: nothing to add, whatever the sum says)
        sample_cell_add(cell, other);
        CHECK(cell.count == 2 && cell.sum == 2.5);
    }

    // walks: rows on instants, several instants inside one interval, gaps, a step back in time, windows
    {
        const int64_t none = INT64_MAX;
        std::vector<Row> rows;
        for (int k = 0; k < 40; k++) rows.push_back(Row{1000 + 100 * k + (k % 7) * 3, (float)(k * k) * 0.25f - 17.0f});
        rows.push_back(Row{2000, 5.0f});  // a step back in time: links nothing
        rows.push_back(Row{2000, 6.0f});  // equal timestamps: count 2 at the instant
        rows.push_back(Row{9000, -1.0f}); // a long interval: many instants inside
        for (uint32_t method : {MDB_SAMPLE_LINEAR, MDB_SAMPLE_STEP, MDB_SAMPLE_EXACT})
            for (int64_t max_gap : {none, (int64_t)0, (int64_t)99, (int64_t)103, (int64_t)118, (int64_t)7000}) {
                check_walk("own grid", rows, 1000, 100, 0, 90, max_gap, method);
                check_walk("narrow", rows, 990, 7, 0, 1200, max_gap, method);
                check_walk("window", rows, 990, 7, 100, 333, max_gap, method);
                check_walk("wide", rows, -5000, 2500, 0, 7, max_gap, method);
                check_walk("behind", rows, 9001, 10, 0, 5, max_gap, method);
                check_walk("before", rows, 0, 10, 0, 100, max_gap, method);
            }
        // at the ends of int64
        const std::vector<Row> ends = {{INT64_MIN, 1.0f}, {INT64_MIN + 10, 3.0f}, {INT64_MAX - 10, -2.0f}, {INT64_MAX, 4.0f}};
        for (uint32_t method : {MDB_SAMPLE_LINEAR, MDB_SAMPLE_STEP, MDB_SAMPLE_EXACT}) {
            check_walk("low end", ends, INT64_MIN, 5, 0, 4, none, method);
            check_walk("both ends", ends, INT64_MIN, INT64_MAX, 0, 3, none, method);
            check_walk("high end", ends, INT64_MAX - 20, 5, 0, 5, none, method);
            check_walk("high end, gap", ends, INT64_MAX - 20, 5, 0, 5, 10, method);
        }
    }

    // merge and values
    {
        mdb_sample_cell into[4] = {{0, 0.0}, {10, 2.5}, {UINT64_MAX - 5, -1.0}, {0, 0.0}};
        const mdb_sample_cell from[4] = {{7, -0.0}, {0, 0.0}, {5, 1.0}, {0, 0.0}};
        CHECK(mdb_sample_merge_n(into, from, 4) == 0);
        CHECK(into[0].count == 7 && into[0].sum == 0.0 && std::signbit(into[0].sum));
        CHECK(into[1].count == 10 && into[1].sum == 2.5 && into[2].count == UINT64_MAX && into[2].sum == 0.0);
        CHECK(into[3].count == 0 && into[3].sum == 0.0 && !std::signbit(into[3].sum));
        double out[3] = {0.0, 0.0, 0.0};
        const mdb_sample_cell cells[3] = {{0, 0.0}, {4, 10.0}, {2, INFINITY}};
        CHECK(mdb_sample_values(cells, 3, out) == 0);
        CHECK(std::isnan(out[0]) && out[1] == 2.5 && std::isinf(out[2]));
        CHECK(mdb_sample_merge_n(nullptr, from, 1) == 1 && mdb_sample_values(cells, 1, nullptr) == 1);
        CHECK(mdb_sample_merge_n(nullptr, nullptr, 0) == 0 && mdb_sample_values(nullptr, 0, nullptr) == 0);
    }

    // malformed requests fail before the device step and leave the cells alone
    {
        mdb_ctx *ctx = reinterpret_cast<mdb_ctx *>(8); // (never dereferenced)
        mdb_segments batch;
        std::memset(&batch, 0, sizeof(batch));
        batch.n = 3;
        const mdb_segments *inputs[1] = {&batch};
        mdb_sample_cell cells[4], before[4];
        std::memset(cells, 0xA5, sizeof(cells));
        std::memcpy(before, cells, sizeof(cells));
        const mdb_sample_request good = {{0, 100, 4, INT64_MIN, INT64_MAX, 1, 0}, INT64_MAX, MDB_SAMPLE_LINEAR, 0};
        struct Bad {
            mdb_sample_request request;
            const char *message;
        };
        std::vector<Bad> bad;
        auto with = [&](auto change, const char *message) {
            mdb_sample_request request = good;
            change(request);
            bad.push_back(Bad{request, message});
        };
        with([](mdb_sample_request &q) { q.instants.which_mask = 1; }, "which_mask");
        with([](mdb_sample_request &q) { q.instants.width = 0; }, "width");
        with([](mdb_sample_request &q) { q.instants.width = -7; }, "width");
        with([](mdb_sample_request &q) { q.instants.n_groups = 0; }, "n_groups must");
        with([](mdb_sample_request &q) { q.instants.n_groups = 4000000000u; q.instants.n_buckets = 1ull << 60; }, "overflows");
        with([](mdb_sample_request &q) { q.instants.t_lo = 0; }, "time range");
        with([](mdb_sample_request &q) { q.instants.t_hi = 1000; }, "time range");
        with([](mdb_sample_request &q) { q.method = 3; }, "method");
        with([](mdb_sample_request &q) { q.flags = 1; }, "flags");
        with([](mdb_sample_request &q) { q.max_gap = -1; }, "max_gap");
        for (const Bad &b : bad) {
            CHECK(mdb_sample_at(ctx, &batch, nullptr, &b.request, cells) == 1);
            CHECK(g_last_error.find(b.message) != std::string::npos);
            CHECK(mdb_sample_at_list(ctx, inputs, nullptr, 1, &b.request, cells) == 1);
            CHECK(g_last_error.find(b.message) != std::string::npos);
        }
        mdb_sample_request every_method = good;
        for (uint32_t method : {MDB_SAMPLE_LINEAR, MDB_SAMPLE_STEP, MDB_SAMPLE_EXACT}) {
            uint64_t n_cells = 0;
            every_method.method = method;
            CHECK(sample_request_check(&every_method, &n_cells) == 0 && n_cells == 4);
        }
        CHECK(mdb_sample_at(nullptr, &batch, nullptr, &good, cells) == 1);
        CHECK(mdb_sample_at(ctx, nullptr, nullptr, &good, cells) == 1);
        CHECK(mdb_sample_at(ctx, &batch, nullptr, nullptr, cells) == 1);
        CHECK(mdb_sample_at(ctx, &batch, nullptr, &good, nullptr) == 1);
        const mdb_segments *missing[1] = {nullptr};
        CHECK(mdb_sample_at_list(ctx, missing, nullptr, 1, &good, cells) == 1);
        CHECK(device_calls == 0);
        CHECK(std::memcmp(cells, before, sizeof(cells)) == 0);
        // nothing to do: success without the device
        mdb_sample_request no_instants = good;
        no_instants.instants.n_buckets = 0;
        CHECK(mdb_sample_at(ctx, &batch, nullptr, &no_instants, cells) == 0);
        CHECK(mdb_sample_at_list(ctx, inputs, nullptr, 0, &good, cells) == 0);
        CHECK(device_calls == 0);
        CHECK(mdb_sample_at(ctx, &batch, nullptr, &good, cells) == 0);
        CHECK(device_calls == 1);
        CHECK(std::memcmp(cells, before, sizeof(cells)) == 0);
    }

    if (failures) {
        std::printf("%d MISMATCH(es)\n", failures);
        return 1;
    }
    std::printf("ok: instants, f(T), walks, merge, values and request checks\n");
    return 0;
}
