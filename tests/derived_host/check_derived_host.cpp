// check_derived_host.cpp - TEST INFRASTRUCTURE: the entry points of the derived-field operator that run before the
// device is needed (mdb_derived_host.cpp), without a GPU. The evaluator is compared with the same formula written out
// here in volatile floats (one rounding per operation), the run arithmetic and mdb_derived_merge_n with long double
// two-pass sums over the same values, and the host forms are handed malformed requests and expressions: they must fail
// with their messages before the device steps - here stand-ins that count their calls - are reached, and leave the
// outputs alone.
#include "../../modelardb-rs_amd/csrc/mdb_derived.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int derived_list_run(mdb_ctx *, const mdb_segments *const *, uint32_t, const mdb_segments *const *, uint32_t,
                     const uint32_t *const *, const mdb_bucket_request *, const mdb_derived_expr *, uint64_t,
                     mdb_derived_cell *) {
    device_calls++;
    return 0;
}
int derived_values_host_run(mdb_ctx *, const mdb_segments *, const mdb_segments *, const mdb_derived_expr *, int64_t,
                            int64_t, int64_t *, float *, uint64_t, uint64_t *) {
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

typedef std::vector<float> Values;

static uint32_t bits_of(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    return bits;
}

// The formula of mdb_format.h, every intermediate stored to a volatile float: one binary32 rounding per operation.
static float written_out(const mdb_derived_expr &e, float x, float y) {
    volatile float z;
    if (e.op == MDB_DERIVED_LINEAR) {
        volatile float ax = e.a * x;
        volatile float by = e.b * y;
        volatile float sum = ax + by;
        z = sum + e.c;
    } else {
        volatile float inner = e.op == MDB_DERIVED_PRODUCT ? x * y : x / y;
        volatile float scaled = e.a * inner;
        z = scaled + e.c;
    }
    float out = z;
    if (e.flags & MDB_DERIVED_ABS) {
        uint32_t bits = bits_of(out) & 0x7fffffffu;
        std::memcpy(&out, &bits, 4);
    }
    return out;
}

static void check_evaluator() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float specials[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-45f, -1e-45f, 1.1754942e-38f, 1.17549435e-38f, 3e-39f, 3.4028235e38f,
                              -3.4028235e38f, inf, -inf, nan, -nan, 0.1f, 3.0f, 1e20f, 1e-20f, 123456.789f};
    const float coefficients[] = {1.0f, -1.0f, 0.0f, -0.0f, 0.1f, 1e-20f, 3.3e7f};
    std::mt19937 rng(2050);
    std::uniform_int_distribution<uint32_t> any_bits;
    Values xs(specials, specials + sizeof(specials) / 4), ys;
    for (int k = 0; k < 100; k++) {
        const uint32_t bits = any_bits(rng);
        float v;
        std::memcpy(&v, &bits, 4);
        xs.push_back(v);
    }
    ys = xs;
    uint64_t compared = 0, denormal_results = 0;
    for (uint32_t op = 0; op <= MDB_DERIVED_RATIO; op++)
        for (uint32_t flags = 0; flags <= MDB_DERIVED_ABS; flags++)
            for (float a : coefficients)
                for (float c : {0.0f, -0.0f, 0.1f}) {
                    const mdb_derived_expr e = {op, flags, a, coefficients[(compared / 7) % 7], c};
                    CHECK(derived_expr_check(&e) == 0);
                    Values z(xs.size());
                    for (float y : ys) {
                        Values repeated(xs.size(), y);
                        CHECK(mdb_derived_apply(&e, xs.data(), repeated.data(), xs.size(), z.data()) == 0);
                        for (size_t k = 0; k < xs.size(); k++) {
                            const float expected = written_out(e, xs[k], y);
                            const bool same = bits_of(z[k]) == bits_of(expected) || (z[k] != z[k] && expected != expected);
                            if (!same) std::printf("op %u flags %u a %g c %g x %a y %a: %a, expected %a\n", op, flags, a, c, xs[k], y, z[k], expected);
                            CHECK(same);
                            if (flags) CHECK((bits_of(z[k]) >> 31) == 0);
                            denormal_results += std::fpclassify(z[k]) == FP_SUBNORMAL;
                            compared++;
                        }
                    }
                }
    CHECK(denormal_results > 0);
    // zeros follow from the formula as written
    const mdb_derived_expr plus = {MDB_DERIVED_LINEAR, 0, 1.0f, 1.0f, 0.0f}, minus = {MDB_DERIVED_LINEAR, 0, 1.0f, 1.0f, -0.0f};
    CHECK(bits_of(derived_eval(plus, -0.0f, -0.0f)) == 0u);
    CHECK(bits_of(derived_eval(minus, -0.0f, -0.0f)) == 0x80000000u);
    const mdb_derived_expr ratio = {MDB_DERIVED_RATIO, 0, 1.0f, 0.0f, 0.0f};
    CHECK(derived_eval(ratio, 0.0f, 0.0f) != derived_eval(ratio, 0.0f, 0.0f)); // 0 / 0
    CHECK(derived_eval(ratio, 1.0f, 0.0f) == inf && derived_eval(ratio, -1.0f, 0.0f) == -inf);
    std::printf("evaluator: %llu values compared, %llu denormal results\n", (unsigned long long)compared,
                (unsigned long long)denormal_results);
}

struct Reference {
    long double mean, m2, largest;
    float min, max;
};
static Reference reference_of(const Values &z) {
    Reference r = {0.0L, 0.0L, 0.0L, FLT_MAX, -FLT_MAX};
    if (z.empty()) return r;
    long double sum = 0.0L;
    for (float v : z) sum += (long double)v - (long double)z[0];
    r.mean = (long double)z[0] + sum / (long double)z.size();
    for (float v : z) {
        const long double d = (long double)v - r.mean;
        r.m2 += d * d;
        r.largest = std::fmax(r.largest, std::fabs((long double)v));
        if (v < r.min) r.min = v;
        if (v > r.max) r.max = v;
    }
    return r;
}

static mdb_derived_cell cell_of(const Values &z) {
    DerivedRun run = derived_run_empty();
    for (float v : z) derived_point(run, v);
    return derived_finish(run);
}

// The tolerances of tests/test_gpu_derived.py: count, min, max exact; 2^-44 of the largest |z| on the mean, 1e-5 of m2.
static bool close_to(const mdb_derived_cell &cell, const Values &z) {
    const Reference r = reference_of(z);
    if (cell.count != (int64_t)z.size()) return false;
    if (z.empty()) return cell.mean == 0.0 && cell.m2 == 0.0 && bits_of(cell.min) == 0 && bits_of(cell.max) == 0;
    return cell.min == r.min && cell.max == r.max && std::fabs((long double)cell.mean - r.mean) <= std::ldexp(r.largest, -44) &&
           std::fabs((long double)cell.m2 - r.m2) <= 1e-5L * r.m2 && cell.m2 >= 0.0;
}

static void check_runs_and_merges() {
    std::mt19937 rng(2051);
    for (double level : {0.0, 1.0e6, 1.0e7}) {
        std::normal_distribution<double> noise(0.0, 0.5);
        Values x(20000), y(20000), z(20000);
        for (size_t k = 0; k < x.size(); k++) x[k] = (float)(level + noise(rng)), y[k] = (float)(level + noise(rng));
        for (uint32_t op = 0; op <= MDB_DERIVED_RATIO; op++) {
            const mdb_derived_expr e = {op, op == MDB_DERIVED_LINEAR ? MDB_DERIVED_ABS : 0u, 1.0f, -1.0f, 0.0f};
            if (op == MDB_DERIVED_RATIO && level == 0.0) continue; // (y near 0: the values are not a data set of the project)
            CHECK(mdb_derived_apply(&e, x.data(), y.data(), x.size(), z.data()) == 0);
            CHECK(close_to(cell_of(z), z));
            for (int n_runs : {2, 29, 400, 2858}) {
                std::vector<size_t> cuts = {0, z.size()};
                std::uniform_int_distribution<size_t> at(0, z.size());
                for (int k = 1; k < n_runs; k++) cuts.push_back(at(rng));
                std::sort(cuts.begin(), cuts.end());
                std::vector<mdb_derived_cell> cells;
                for (size_t k = 0; k + 1 < cuts.size(); k++) cells.push_back(cell_of(Values(z.begin() + cuts[k], z.begin() + cuts[k + 1])));
                mdb_derived_cell forward = {0, 0.0, 0.0, 0.0f, 0.0f}, backward = forward;
                for (size_t k = 0; k < cells.size(); k++) {
                    CHECK(mdb_derived_merge_n(&forward, &cells[k], 1) == 0);
                    CHECK(mdb_derived_merge_n(&backward, &cells[cells.size() - 1 - k], 1) == 0);
                }
                CHECK(close_to(forward, z));
                CHECK(close_to(backward, z));
                CHECK(forward.count == backward.count && forward.min == backward.min && forward.max == backward.max);
            }
        }
    }
    // all z equal: m2 == 0.0 and mean == z exactly, in any order of merges
    const Values equal(777, 1234.567f);
    mdb_derived_cell into = cell_of(Values(equal.begin(), equal.begin() + 5));
    const mdb_derived_cell rest = cell_of(Values(equal.begin() + 5, equal.end())), one = cell_of(Values(1, 1234.567f));
    mdb_derived_merge_n(&into, &rest, 1);
    for (int k = 0; k < 100; k++) mdb_derived_merge_n(&into, &one, 1);
    CHECK(into.count == 877 && into.m2 == 0.0 && into.mean == (double)1234.567f && into.min == 1234.567f && into.max == 1234.567f);
    // NaNs are skipped by min and max; a cell of NaNs only keeps FLT_MAX / -FLT_MAX
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const mdb_derived_cell nans = cell_of(Values{nan, nan}), mixed = cell_of(Values{nan, 2.0f, -3.0f, nan});
    CHECK(nans.count == 2 && nans.min == FLT_MAX && nans.max == -FLT_MAX && nans.mean != nans.mean);
    CHECK(mixed.count == 4 && mixed.min == -3.0f && mixed.max == 2.0f);
    mdb_derived_cell merged = nans;
    mdb_derived_merge_n(&merged, &mixed, 1);
    CHECK(merged.count == 6 && merged.min == -3.0f && merged.max == 2.0f);
    // an empty side gives the other side's bytes; count 0 reads nothing
    mdb_derived_cell stale;
    std::memset(&stale, 0xA5, sizeof stale);
    stale.count = 0;
    mdb_derived_cell copy = stale;
    const mdb_derived_cell fresh = {0, 0.0, 0.0, 0.0f, 0.0f};
    mdb_derived_merge_n(&copy, &fresh, 1);
    CHECK(std::memcmp(&copy, &stale, sizeof copy) == 0);
    mdb_derived_merge_n(&copy, &mixed, 1);
    CHECK(std::memcmp(&copy, &mixed, sizeof copy) == 0);
    mdb_derived_merge_n(&copy, &stale, 1);
    CHECK(std::memcmp(&copy, &mixed, sizeof copy) == 0);
    // mdb_derived_stats
    const mdb_derived_cell three[3] = {mixed, stale, one};
    mdb_moments_cell out[3];
    std::memset(out, 0x11, sizeof out);
    CHECK(mdb_derived_stats(three, 3, out) == 0);
    CHECK(out[0].count == 4 && out[1].count == 0 && out[1].mean == 0.0 && out[1].m2 == 0.0 && out[2].count == 1 && out[2].m2 == 0.0);
    CHECK(mdb_derived_stats(nullptr, 1, out) == 1 && mdb_derived_stats(three, 1, nullptr) == 1 && mdb_derived_stats(nullptr, 0, nullptr) == 0);
    CHECK(mdb_derived_merge_n(nullptr, three, 1) == 1 && mdb_derived_merge_n(nullptr, nullptr, 0) == 0);
}

static void check_requests() {
    mdb_ctx *fake = reinterpret_cast<mdb_ctx *>(8); // (never dereferenced)
    mdb_segments batch;
    std::memset(&batch, 0, sizeof batch);
    batch.n = 1;
    const mdb_segments *list[1] = {&batch};
    std::vector<mdb_derived_cell> cells(4);
    std::memset(cells.data(), 0xA5, 4 * sizeof(mdb_derived_cell));
    const std::vector<mdb_derived_cell> before = cells;
    const mdb_derived_expr good = {MDB_DERIVED_PRODUCT, 0, 1.0f, 0.0f, 0.0f};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const mdb_bucket_request ok = {0, 100, 4, INT64_MIN, INT64_MAX, 1, 0};
    const mdb_bucket_request bad_requests[] = {{0, 100, 4, INT64_MIN, INT64_MAX, 1, 1}, {0, 0, 4, INT64_MIN, INT64_MAX, 1, 0},
                                               {0, 100, 4, INT64_MIN, INT64_MAX, 0, 0},
                                               {0, 100, UINT64_MAX / 8, INT64_MIN, INT64_MAX, 4000000000u, 0}};
    const mdb_derived_expr bad_exprs[] = {{3, 0, 1.0f, 1.0f, 0.0f}, {0, 2, 1.0f, 1.0f, 0.0f}, {0, 0, nan, 1.0f, 0.0f},
                                          {1, 0, 1.0f, inf, 0.0f}, {2, 1, 1.0f, 1.0f, -inf}};
    float values[4] = {7.0f, 7.0f, 7.0f, 7.0f};
    uint64_t rows = 99;
    for (const mdb_bucket_request &request : bad_requests) {
        CHECK(mdb_derived_buckets(fake, &batch, &batch, nullptr, &request, &good, cells.data()) == 1);
        CHECK(mdb_derived_buckets_list(fake, list, 1, list, 1, nullptr, &request, &good, cells.data()) == 1);
    }
    for (const mdb_derived_expr &expr : bad_exprs) {
        CHECK(mdb_derived_buckets(fake, &batch, &batch, nullptr, &ok, &expr, cells.data()) == 1);
        CHECK(mdb_derived_buckets_list(fake, list, 1, list, 1, nullptr, &ok, &expr, cells.data()) == 1);
        CHECK(mdb_derived_values(fake, &batch, &batch, &expr, INT64_MIN, INT64_MAX, nullptr, values, 4, &rows) == 1);
        CHECK(mdb_derived_apply(&expr, values, values, 4, values) == 1);
    }
    CHECK(mdb_derived_buckets(fake, &batch, nullptr, nullptr, &ok, &good, cells.data()) == 1);
    CHECK(mdb_derived_buckets(fake, &batch, &batch, nullptr, &ok, nullptr, cells.data()) == 1);
    CHECK(mdb_derived_buckets(nullptr, &batch, &batch, nullptr, &ok, &good, cells.data()) == 1);
    CHECK(mdb_derived_buckets_list(fake, list, 1, nullptr, 1, nullptr, &ok, &good, cells.data()) == 1);
    CHECK(mdb_derived_values(fake, &batch, nullptr, &good, 0, 1, nullptr, values, 4, &rows) == 1);
    CHECK(mdb_derived_values(fake, &batch, &batch, &good, 0, 1, nullptr, values, 4, nullptr) == 1);
    CHECK(device_calls == 0 && rows == 99 && values[0] == 7.0f && values[3] == 7.0f);
    CHECK(std::memcmp(cells.data(), before.data(), 4 * sizeof(mdb_derived_cell)) == 0);
    // an empty range, an empty batch, no buckets: success without the device
    CHECK(mdb_derived_values(fake, &batch, &batch, &good, 5, 4, nullptr, values, 4, &rows) == 0 && rows == 0);
    batch.n = 0;
    rows = 99;
    CHECK(mdb_derived_values(fake, &batch, &batch, &good, 0, 1, nullptr, values, 4, &rows) == 0 && rows == 0);
    CHECK(mdb_derived_buckets(fake, &batch, &batch, nullptr, &ok, &good, cells.data()) == 0);
    batch.n = 1;
    const mdb_bucket_request none = {0, 100, 0, INT64_MIN, INT64_MAX, 1, 0};
    CHECK(mdb_derived_buckets(fake, &batch, &batch, nullptr, &none, &good, cells.data()) == 0);
    CHECK(device_calls == 0);
    CHECK(std::memcmp(cells.data(), before.data(), 4 * sizeof(mdb_derived_cell)) == 0);
    // and a good call reaches the device step
    CHECK(mdb_derived_buckets(fake, &batch, &batch, nullptr, &ok, &good, cells.data()) == 0 && device_calls == 1);
    CHECK(mdb_derived_values(fake, &batch, &batch, &good, 0, 1, nullptr, values, 4, &rows) == 0 && device_calls == 2);
}

int main() {
    check_evaluator();
    check_runs_and_merges();
    check_requests();
    if (failures) {
        std::printf("%d MISMATCH(es)\n", failures);
        return 1;
    }
    std::printf("ok: the evaluator, the run arithmetic, the merge rule and the checks of the derived-field operator\n");
    return 0;
}
