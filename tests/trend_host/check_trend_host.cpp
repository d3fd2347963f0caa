// check_trend_host.cpp - TEST INFRASTRUCTURE: the part of the trend operator that needs no GPU. The closed forms of
// mdb_trend.hpp (the x side of n points on regular timestamps, the PMC-Mean cell, the Swing cell) and the run of
// trend_point are compared with long double sums over the same points, and the host forms (mdb_trend_host.cpp) are
// handed malformed requests: they must fail with their messages before trend_list_run - here a stand-in that counts
// its calls - is reached, and leave the cells alone.
#include "../../modelardb-rs_amd/csrc/mdb_trend.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int trend_list_run(mdb_ctx *, const mdb_segments *const *, const uint32_t *const *, uint32_t, const mdb_bucket_request *,
                   uint64_t, mdb_comoments_cell *) {
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

// mean and m2 of x0 + k * delta, k < n, point by point. Exact in integers: with d_k = 2k - (n-1) (twice the distance
// from the mean, an integer) the mean is x0 + delta * (n-1)/2 and m2 = delta^2 * sum(d_k^2) / 4; the sum stays below
// 2^98 and is accumulated in 128 bits, one term a point. The conversions to long double round once each.
struct XSide {
    long double mean, m2;
};
static XSide x_side_point_by_point(uint64_t n, long double x0, long double delta) {
    unsigned __int128 sum = 0;
    const int64_t last = (int64_t)n - 1;
    for (int64_t k = 0; k <= last; k++) {
        const int64_t d = 2 * k - last;
        sum += (unsigned __int128)((__int128)d * d);
    }
    const long double squares = std::ldexp((long double)(uint64_t)(sum >> 64), 64) + (long double)(uint64_t)sum;
    return XSide{x0 + delta * (long double)last / 2.0L, delta * delta * squares / 4.0L};
}

// A tolerance far inside the tests' (2^-44 of the largest |x| on a mean, 1e-5 on m2): the closed forms round a
// handful of times.
static bool x_side_close(double mean, double m2, const XSide &r, long double largest) {
    return std::fabs((long double)mean - r.mean) <= std::ldexp(largest, -50) &&
           std::fabs((long double)m2 - r.m2) <= std::ldexp(r.m2, -48) && m2 >= 0.0;
}

int main() {
    // the x side: n in {1, 2, 7, 64, 745, 2^32 - 1}, delta in {1, 100, 2^40}, x0 at 0 and just below a width of 2^52
    const uint64_t counts[] = {1, 2, 7, 64, 745, 0xffffffffull};
    const double deltas[] = {1.0, 100.0, 1099511627776.0};
    const double firsts[] = {0.0, 4503599627370495.0};
    XSide unit[6];
    for (int c = 0; c < 6; c++) unit[c] = x_side_point_by_point(counts[c], 0.0L, 1.0L); // (the long loop once)
    for (int c = 0; c < 6; c++) {
        const uint64_t n = counts[c];
        for (double delta : deltas) {
            for (double x0 : firsts) {
                const XSide reference = {(long double)x0 + (long double)delta * unit[c].mean,
                                         (long double)delta * (long double)delta * unit[c].m2};
                if (n <= 745) { // (and once more from the points themselves)
                    const XSide again = x_side_point_by_point(n, (long double)x0, (long double)delta);
                    CHECK(again.mean == reference.mean && std::fabs(again.m2 - reference.m2) <= std::ldexp(reference.m2, -60));
                    long double sum = 0.0L, m2 = 0.0L;
                    for (uint64_t k = 0; k < n; k++) sum += (long double)k * (long double)delta;
                    const long double mean = (long double)x0 + sum / (long double)n;
                    for (uint64_t k = 0; k < n; k++) {
                        const long double d = (long double)x0 + (long double)k * (long double)delta - mean;
                        m2 += d * d;
                    }
                    CHECK(std::fabs(mean - reference.mean) <= std::ldexp(std::fabs(reference.mean), -60));
                    CHECK(std::fabs(m2 - reference.m2) <= std::ldexp(reference.m2, -50));
                }
                const long double largest = (long double)x0 + (long double)delta * (long double)(n - 1);
                double mean_x = -1.0, m2_x = -1.0;
                trend_regular_x(n, x0, delta, &mean_x, &m2_x);
                CHECK(x_side_close(mean_x, m2_x, reference, largest));
                if (n == 1) CHECK(mean_x == x0 && m2_x == 0.0);
                CHECK(std::fabs((long double)(delta * trend_index_sum(n)) -
                                (long double)delta * (long double)(n - 1) * (long double)n / 2.0L) <=
                      std::ldexp((long double)delta * (long double)n * (long double)n, -52));
                // the PMC-Mean cell: a finite, an infinite and a NaN value
                const mdb_comoments_cell flat = trend_constant_cell(n, x0, delta, 1234.567f);
                CHECK(flat.count == (int64_t)n && flat.mean_x == mean_x && flat.m2_x == m2_x);
                CHECK(flat.mean_y == (double)1234.567f && flat.m2_y == 0.0 && flat.c_xy == 0.0);
                for (float special : {INFINITY, -INFINITY, NAN}) {
                    const mdb_comoments_cell cell = trend_constant_cell(n, x0, delta, special);
                    CHECK(cell.count == (int64_t)n && cell.mean_x == mean_x && cell.m2_x == m2_x);
                    CHECK(!std::isfinite(cell.mean_y) && std::isnan(cell.m2_y) && std::isnan(cell.c_xy));
                }
            }
        }
    }
    CHECK(trend_constant_cell(0, 5.0, 100.0, 1.0f).count == 0);
    // every point at one instant (delta 0): m2_x is 0.0 exactly
    {
        double mean_x = -1.0, m2_x = -1.0;
        trend_regular_x(1000, 777.0, 0.0, &mean_x, &m2_x);
        CHECK(mean_x == 777.0 && m2_x == 0.0);
    }

    // a run of trend_point and the Swing cell (x side closed, y side summed) against long double two-pass sums, at
    // bucket bases near both ends of int64 and at epoch scale
    std::mt19937_64 rng(20261019);
    std::normal_distribution<double> noise(0.0, 0.5);
    const int64_t origins[] = {0, 1658671178037000LL, INT64_MIN + 5, INT64_MAX - (1LL << 41)};
    for (int64_t origin : origins) {
        for (size_t n : {(size_t)1, (size_t)2, (size_t)7, (size_t)64, (size_t)745}) {
            for (int64_t delta : {(int64_t)1, (int64_t)100, (int64_t)1 << 30}) {
                const int64_t width = (int64_t)1 << 41;
                const uint64_t base = trend_bucket_base(origin, width, 0);
                const int64_t t0 = (int64_t)(base + 12345u);
                std::vector<float> values(n);
                for (size_t k = 0; k < n; k++) values[k] = (float)(1.0e6 + 0.01 * (double)k + noise(rng));
                TrendRun run = trend_run_empty();
                double sy = 0.0, syy = 0.0, sxy = 0.0;
                for (size_t k = 0; k < n; k++) {
                    const int64_t t = (int64_t)((uint64_t)t0 + (uint64_t)k * (uint64_t)delta);
                    CHECK(trend_x(t, base) == 12345.0 + (double)k * (double)delta);
                    trend_point(run, base, t, values[k]);
                    const double dy = (double)values[k] - (double)values[0], dx = (double)((uint64_t)k * (uint64_t)delta);
                    sy += dy, syy += dy * dy, sxy += dx * dy;
                }
                const mdb_comoments_cell summed = trend_finish(run);
                const mdb_comoments_cell closed = trend_regular_cell(n, 12345.0, (double)delta, (double)values[0], sy, syy, sxy);
                long double sum_x = 0.0L, sum_y = 0.0L, largest_y = 0.0L;
                for (size_t k = 0; k < n; k++) {
                    sum_x += (long double)k * (long double)delta;
                    sum_y += (long double)values[k] - (long double)values[0];
                    largest_y = std::fmax(largest_y, std::fabs((long double)values[k]));
                }
                const long double mean_x = 12345.0L + sum_x / (long double)n, mean_y = (long double)values[0] + sum_y / (long double)n;
                long double m2_x = 0.0L, m2_y = 0.0L, c = 0.0L;
                for (size_t k = 0; k < n; k++) {
                    const long double dx = 12345.0L + (long double)k * (long double)delta - mean_x, dy = (long double)values[k] - mean_y;
                    m2_x += dx * dx, m2_y += dy * dy, c += dx * dy;
                }
                const long double largest_x = 12345.0L + (long double)(n - 1) * (long double)delta;
                for (const mdb_comoments_cell &cell : {summed, closed}) {
                    CHECK(cell.count == (int64_t)n);
                    CHECK(std::fabs((long double)cell.mean_x - mean_x) <= std::ldexp(largest_x, -44));
                    CHECK(std::fabs((long double)cell.mean_y - mean_y) <= std::ldexp(largest_y, -44));
                    CHECK(std::fabs((long double)cell.m2_x - m2_x) <= 1e-5L * m2_x && cell.m2_x >= 0.0);
                    CHECK(std::fabs((long double)cell.m2_y - m2_y) <= 1e-5L * m2_y && cell.m2_y >= 0.0);
                    CHECK(std::fabs((long double)cell.c_xy - c) <= 1e-5L * std::sqrt(m2_x * m2_y));
                }
                if (n == 1) CHECK(summed.m2_x == 0.0 && summed.c_xy == 0.0 && closed.m2_x == 0.0 && closed.c_xy == 0.0);
            }
        }
    }
    // equal values: m2_y and c_xy are 0.0 exactly; a NaN leaves the x side alone
    {
        TrendRun flat = trend_run_empty(), broken = trend_run_empty();
        for (int k = 0; k < 50; k++) {
            trend_point(flat, 1000, 1000 + 7 * k, 3.25f);
            trend_point(broken, 1000, 1000 + 7 * k, k == 20 ? NAN : 3.25f);
        }
        const mdb_comoments_cell a = trend_finish(flat), b = trend_finish(broken);
        CHECK(a.m2_y == 0.0 && a.c_xy == 0.0 && a.m2_x > 0.0 && a.mean_y == 3.25);
        CHECK(b.count == 50 && b.mean_x == a.mean_x && b.m2_x == a.m2_x);
        CHECK(std::isnan(b.mean_y) && std::isnan(b.m2_y) && std::isnan(b.c_xy));
        CHECK(comoments_statistic(a, MDB_COMOMENTS_REGR_SLOPE) == 0.0 && std::isnan(comoments_statistic(a, MDB_COMOMENTS_CORR)));
        // all points at one timestamp: no slope
        TrendRun instant = trend_run_empty();
        for (int k = 0; k < 5; k++) trend_point(instant, 1000, 1400, (float)k);
        const mdb_comoments_cell c = trend_finish(instant);
        CHECK(c.m2_x == 0.0 && c.mean_x == 400.0 && c.m2_y > 0.0 && std::isnan(comoments_statistic(c, MDB_COMOMENTS_REGR_SLOPE)));
        CHECK(trend_finish(trend_run_empty()).count == 0);
    }

    // the host forms: malformed requests fail before the device step, with the messages of mdb_moments_buckets
    mdb_ctx *fake_context = reinterpret_cast<mdb_ctx *>(8); // (never dereferenced)
    mdb_segments batch;
    std::memset(&batch, 0, sizeof batch);
    batch.n = 1;
    const mdb_segments *inputs[1] = {&batch};
    const mdb_segments *with_null[1] = {nullptr};
    mdb_comoments_cell cells[4];
    std::memset(cells, 0xA5, sizeof cells);
    struct Bad {
        mdb_bucket_request request;
        const char *message;
    };
    const Bad bad[] = {{{0, 100, 4, INT64_MIN, INT64_MAX, 1, 1}, "which_mask must be 0 for mdb_trend_buckets*."},
                       {{0, 0, 4, INT64_MIN, INT64_MAX, 1, 0}, "The bucket width must be positive."},
                       {{0, -7, 4, INT64_MIN, INT64_MAX, 1, 0}, "The bucket width must be positive."},
                       {{0, 100, 4, INT64_MIN, INT64_MAX, 0, 0}, "n_groups must be at least 1."},
                       {{0, 100, UINT64_MAX / 8, INT64_MIN, INT64_MAX, 4000000000u, 0}, "n_groups * n_buckets overflows."}};
    for (const Bad &b : bad) {
        CHECK(mdb_trend_buckets_list(fake_context, inputs, nullptr, 1, &b.request, cells) == 1 && g_last_error == b.message);
        g_last_error.clear();
        CHECK(mdb_trend_buckets(fake_context, &batch, nullptr, &b.request, cells) == 1 && g_last_error == b.message);
    }
    const mdb_bucket_request good = {0, 100, 4, INT64_MIN, INT64_MAX, 1, 0}, no_buckets = {0, 100, 0, INT64_MIN, INT64_MAX, 1, 0};
    CHECK(mdb_trend_buckets_list(nullptr, inputs, nullptr, 1, &good, cells) == 1 && g_last_error.find("NULL") != std::string::npos);
    CHECK(mdb_trend_buckets_list(fake_context, nullptr, nullptr, 1, &good, cells) == 1);
    CHECK(mdb_trend_buckets_list(fake_context, inputs, nullptr, 1, nullptr, cells) == 1);
    CHECK(mdb_trend_buckets_list(fake_context, inputs, nullptr, 1, &good, nullptr) == 1);
    CHECK(mdb_trend_buckets(fake_context, nullptr, nullptr, &good, cells) == 1 && g_last_error.find("NULL") != std::string::npos);
    CHECK(mdb_trend_buckets_list(fake_context, with_null, nullptr, 1, &good, cells) == 1 && g_last_error == "A batch of the list is NULL.");
    CHECK(device_calls == 0);
    // nothing to do: success without the device
    batch.n = 0;
    CHECK(mdb_trend_buckets_list(fake_context, inputs, nullptr, 1, &good, cells) == 0);
    CHECK(mdb_trend_buckets_list(fake_context, inputs, nullptr, 0, &good, cells) == 0);
    CHECK(mdb_trend_buckets(fake_context, &batch, nullptr, &good, cells) == 0);
    batch.n = 1;
    CHECK(mdb_trend_buckets_list(fake_context, inputs, nullptr, 1, &no_buckets, cells) == 0 && device_calls == 0);
    CHECK(mdb_trend_buckets(fake_context, &batch, nullptr, &good, cells) == 0 && device_calls == 1);
    for (const mdb_comoments_cell &cell : cells) {
        mdb_comoments_cell untouched;
        std::memset(&untouched, 0xA5, sizeof untouched);
        CHECK(std::memcmp(&cell, &untouched, sizeof cell) == 0);
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("ok: closed forms, runs and host forms of the trend operator\n");
    return 0;
}
