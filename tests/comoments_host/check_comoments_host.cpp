// check_comoments_host.cpp - TEST INFRASTRUCTURE: the entry points of the covariance operator that run before the
// device is needed (mdb_comoments_host.cpp), without a GPU. The shifted sums of a run and mdb_comoments_merge_n are
// compared with long double two-pass sums over the same pairs, mdb_comoments_finish and mdb_comoments_moments with
// their definitions, and the host forms are handed malformed requests: they must fail with their messages before
// comoments_list_run - here a stand-in that counts its calls - is reached, and leave the cells alone.
#include "../../modelardb-rs_amd/csrc/mdb_comoments.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int comoments_list_run(mdb_ctx *, const mdb_segments *const *, uint32_t, const mdb_segments *const *, uint32_t,
                       const uint32_t *const *, const mdb_bucket_request *, uint64_t, mdb_comoments_cell *) {
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

typedef std::vector<float> Points;

// The means, m2 and c of the pairs in two passes of long double: the reference of this program.
struct Reference {
    long double mean_x, mean_y, m2_x, m2_y, c, largest_x, largest_y;
};
static Reference reference_of(const Points &x, const Points &y) {
    Reference r = {0.0L, 0.0L, 0.0L, 0.0L, 0.0L, 0.0L, 0.0L};
    if (x.empty()) return r;
    long double sum_x = 0.0L, sum_y = 0.0L;
    for (size_t k = 0; k < x.size(); k++) {
        sum_x += (long double)x[k] - (long double)x[0];
        sum_y += (long double)y[k] - (long double)y[0];
    }
    r.mean_x = (long double)x[0] + sum_x / (long double)x.size();
    r.mean_y = (long double)y[0] + sum_y / (long double)x.size();
    for (size_t k = 0; k < x.size(); k++) {
        const long double dx = (long double)x[k] - r.mean_x, dy = (long double)y[k] - r.mean_y;
        r.m2_x += dx * dx;
        r.m2_y += dy * dy;
        r.c += dx * dy;
        r.largest_x = std::fmax(r.largest_x, std::fabs((long double)x[k]));
        r.largest_y = std::fmax(r.largest_y, std::fabs((long double)y[k]));
    }
    return r;
}

static mdb_comoments_cell cell_of(const Points &x, const Points &y) {
    ComomentsRun run = comoments_run_empty();
    for (size_t k = 0; k < x.size(); k++) comoments_point(run, x[k], y[k]);
    return comoments_finish(run);
}

// The tolerances of tests/test_gpu_comoments.py: 2^-44 of the largest |v| on a mean, 1e-5 of m2 on m2 (0: exactly 0),
// 1e-5 of sqrt(m2_x * m2_y) - the Cauchy-Schwarz bound of |c| - on c_xy.
static bool close_to(const mdb_comoments_cell &cell, const Points &x, const Points &y) {
    const Reference r = reference_of(x, y);
    if (cell.count != (int64_t)x.size()) return false;
    if (x.empty()) return cell.mean_x == 0.0 && cell.m2_x == 0.0 && cell.c_xy == 0.0;
    return std::fabs((long double)cell.mean_x - r.mean_x) <= std::ldexp(r.largest_x, -44) &&
           std::fabs((long double)cell.mean_y - r.mean_y) <= std::ldexp(r.largest_y, -44) &&
           std::fabs((long double)cell.m2_x - r.m2_x) <= 1e-5L * r.m2_x && cell.m2_x >= 0.0 &&
           std::fabs((long double)cell.m2_y - r.m2_y) <= 1e-5L * r.m2_y && cell.m2_y >= 0.0 &&
           std::fabs((long double)cell.c_xy - r.c) <= 1e-5L * std::sqrt(r.m2_x * r.m2_y);
}

static Points part(const Points &points, size_t a, size_t b) { return Points(points.begin() + a, points.begin() + b); }

int main() {
    std::mt19937_64 rng(20261019);
    std::normal_distribution<double> noise(0.0, 0.5);
    // pairs: levels 0, 1e6 and 1e7 with sigma 0.5; y correlated with, anticorrelated with or independent of x; a
    // constant y
    auto data_set = [&](int level_index, int relation, size_t n, Points *x, Points *y) {
        const double level = level_index == 0 ? 0.0 : level_index == 1 ? 1.0e6 : 1.0e7;
        x->resize(n);
        y->resize(n);
        for (size_t k = 0; k < n; k++) {
            const double e = noise(rng), f = noise(rng);
            (*x)[k] = (float)(level + e);
            switch (relation) {
            case 0: (*y)[k] = (float)(level + 0.8 * e + 0.2 * f); break;
            case 1: (*y)[k] = (float)(level - 0.8 * e + 0.2 * f); break;
            case 2: (*y)[k] = (float)(level + f); break;
            default: (*y)[k] = 1234.567f; break;
            }
        }
    };
    for (int level = 0; level < 3; level++) {
        for (int relation = 0; relation < 4; relation++) {
            Points x, y;
            data_set(level, relation, 20000, &x, &y);
            CHECK(close_to(cell_of(x, y), x, y)); // one run
            for (size_t run_length : {(size_t)1, (size_t)7, (size_t)50, (size_t)745}) {
                // runs of run_length merged one after the other, and through tiles of 64 as the reduction tree does
                std::vector<mdb_comoments_cell> runs;
                for (size_t a = 0; a < x.size(); a += run_length) {
                    const size_t b = std::min(x.size(), a + run_length);
                    runs.push_back(cell_of(part(x, a, b), part(y, a, b)));
                }
                mdb_comoments_cell chain = {0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (const mdb_comoments_cell &run : runs) CHECK(mdb_comoments_merge_n(&chain, &run, 1) == 0);
                CHECK(close_to(chain, x, y));
                std::vector<mdb_comoments_cell> tiles = runs;
                while (tiles.size() > 1) {
                    std::vector<mdb_comoments_cell> up;
                    for (size_t a = 0; a < tiles.size(); a += 64) {
                        const size_t b = std::min(tiles.size(), a + 64);
                        mdb_comoments_cell acc = tiles[b - 1];
                        for (size_t t = b - 1; t > a; t--) comoments_merge(acc, tiles[t - 1]);
                        up.push_back(acc);
                    }
                    tiles = up;
                }
                CHECK(close_to(tiles[0], x, y));
                if (relation == 3) // a constant field: c_xy and its m2 are 0.0 exactly, in any order of merges
                    CHECK(chain.c_xy == 0.0 && tiles[0].c_xy == 0.0 && chain.m2_y == 0.0 && tiles[0].m2_y == 0.0 &&
                          chain.mean_y == (double)1234.567f && tiles[0].mean_y == (double)1234.567f);
                // identical fields: m2_x, m2_y and c_xy of the same bytes
                mdb_comoments_cell self = {0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (size_t a = 0; a < x.size(); a += run_length) {
                    const size_t b = std::min(x.size(), a + run_length);
                    const mdb_comoments_cell run = cell_of(part(x, a, b), part(x, a, b));
                    CHECK(mdb_comoments_merge_n(&self, &run, 1) == 0);
                }
                CHECK(std::memcmp(&self.m2_x, &self.m2_y, 8) == 0 && std::memcmp(&self.m2_x, &self.c_xy, 8) == 0 &&
                      self.mean_x == self.mean_y);
                double corr = 0.0;
                CHECK(mdb_comoments_finish(&self, 1, MDB_COMOMENTS_CORR, &corr) == 0 && corr == 1.0);
            }
        }
    }
    // random splits of small sets, merged in both orders
    for (int trial = 0; trial < 2000; trial++) {
        Points x, y;
        data_set((int)(rng() % 3), (int)(rng() % 4), rng() % 40, &x, &y);
        const size_t cut = x.empty() ? 0 : rng() % (x.size() + 1);
        const mdb_comoments_cell a = cell_of(part(x, 0, cut), part(y, 0, cut)), b = cell_of(part(x, cut, x.size()), part(y, cut, y.size()));
        mdb_comoments_cell into[2] = {a, b};
        const mdb_comoments_cell from[2] = {b, a};
        CHECK(mdb_comoments_merge_n(into, from, 2) == 0);
        CHECK(close_to(into[0], x, y) && close_to(into[1], x, y));
    }
    // non-finite points in one field: the count is exact, that field's mean and m2 and c_xy are not finite
    const float specials[] = {NAN, INFINITY, -INFINITY};
    for (float special : specials) {
        for (size_t position : {(size_t)0, (size_t)3, (size_t)9}) {
            Points x, y;
            data_set(0, 2, 10, &x, &y);
            y[position] = special;
            const mdb_comoments_cell one = cell_of(x, y);
            CHECK(one.count == 10 && !std::isfinite(one.mean_y) && !std::isfinite(one.m2_y) && !std::isfinite(one.c_xy));
            CHECK(std::isfinite(one.mean_x) && std::isfinite(one.m2_x));
            Points u, v;
            data_set(1, 0, 5, &u, &v);
            mdb_comoments_cell left = cell_of(u, v), right = one;
            const mdb_comoments_cell finite = left;
            CHECK(mdb_comoments_merge_n(&left, &one, 1) == 0 && mdb_comoments_merge_n(&right, &finite, 1) == 0);
            CHECK(left.count == 15 && !std::isfinite(left.mean_y) && !std::isfinite(left.m2_y) && !std::isfinite(left.c_xy));
            CHECK(right.count == 15 && !std::isfinite(right.mean_y) && !std::isfinite(right.m2_y) && !std::isfinite(right.c_xy));
        }
    }
    // an empty `from` keeps every byte of `into`, also of an empty one; an empty `into` takes `from`'s bytes
    Points x4, y4;
    data_set(1, 0, 4, &x4, &y4);
    mdb_comoments_cell pattern, empty, some = cell_of(x4, y4);
    std::memset(&pattern, 0xA5, sizeof pattern);
    std::memset(&empty, 0, sizeof empty);
    pattern.count = 0;
    mdb_comoments_cell kept = pattern;
    CHECK(mdb_comoments_merge_n(&kept, &empty, 1) == 0 && std::memcmp(&kept, &pattern, sizeof pattern) == 0);
    CHECK(mdb_comoments_merge_n(&kept, &some, 1) == 0 && std::memcmp(&kept, &some, sizeof some) == 0);
    CHECK(mdb_comoments_merge_n(&kept, &empty, 1) == 0 && std::memcmp(&kept, &some, sizeof some) == 0);
    CHECK(mdb_comoments_merge_n(nullptr, nullptr, 0) == 0 && mdb_comoments_merge_n(nullptr, &some, 1) == 1 &&
          mdb_comoments_merge_n(&kept, nullptr, 1) == 1);

    // mdb_comoments_finish: the six kinds and their NaN cases; mdb_comoments_moments: either triple
    const mdb_comoments_cell few[5] = {{0, 9.0, 9.0, 9.0, 9.0, 9.0},  // empty: no other member is read
                                       {1, 5.0, 6.0, 0.0, 0.0, 0.0},
                                       {4, 1.0, 10.0, 8.0, 2.0, -3.0},
                                       {4, 1.0, 10.0, 0.0, 2.0, 0.0},   // x constant
                                       {4, 1.0, 10.0, 8.0, 0.0, 0.0}};  // y constant
    double out[5];
    CHECK(mdb_comoments_finish(few, 5, MDB_COMOMENTS_COVAR_POP, out) == 0);
    CHECK(std::isnan(out[0]) && out[1] == 0.0 && out[2] == -0.75 && out[3] == 0.0 && out[4] == 0.0);
    CHECK(mdb_comoments_finish(few, 5, MDB_COMOMENTS_COVAR_SAMP, out) == 0);
    CHECK(std::isnan(out[0]) && std::isnan(out[1]) && out[2] == -1.0 && out[3] == 0.0);
    CHECK(mdb_comoments_finish(few, 5, MDB_COMOMENTS_CORR, out) == 0);
    CHECK(std::isnan(out[0]) && std::isnan(out[1]) && out[2] == -0.75 && std::isnan(out[3]) && std::isnan(out[4]));
    CHECK(mdb_comoments_finish(few, 5, MDB_COMOMENTS_REGR_SLOPE, out) == 0);
    CHECK(std::isnan(out[0]) && std::isnan(out[1]) && out[2] == -0.375 && std::isnan(out[3]) && out[4] == 0.0);
    CHECK(mdb_comoments_finish(few, 5, MDB_COMOMENTS_REGR_INTERCEPT, out) == 0);
    CHECK(std::isnan(out[0]) && std::isnan(out[1]) && out[2] == 10.375 && std::isnan(out[3]) && out[4] == 10.0);
    CHECK(mdb_comoments_finish(few, 5, MDB_COMOMENTS_REGR_R2, out) == 0);
    CHECK(std::isnan(out[0]) && std::isnan(out[1]) && out[2] == 0.5625 && std::isnan(out[3]) && std::isnan(out[4]));
    out[0] = 77.0;
    CHECK(mdb_comoments_finish(few, 5, 6, out) == 1 && g_last_error.find("kind") != std::string::npos && out[0] == 77.0);
    CHECK(mdb_comoments_finish(nullptr, 0, 0, nullptr) == 0 && mdb_comoments_finish(nullptr, 1, 0, out) == 1 &&
          mdb_comoments_finish(few, 1, 0, nullptr) == 1);
    mdb_moments_cell triple[5];
    CHECK(mdb_comoments_moments(few, 5, 0, triple) == 0);
    CHECK(triple[0].count == 0 && triple[0].mean == 0.0 && triple[0].m2 == 0.0 && triple[2].count == 4 && triple[2].mean == 1.0 && triple[2].m2 == 8.0);
    CHECK(mdb_comoments_moments(few, 5, 1, triple) == 0);
    CHECK(triple[2].count == 4 && triple[2].mean == 10.0 && triple[2].m2 == 2.0);
    CHECK(mdb_comoments_moments(few, 5, 2, triple) == 1 && g_last_error.find("which") != std::string::npos);
    CHECK(mdb_comoments_moments(nullptr, 1, 0, triple) == 1 && mdb_comoments_moments(few, 1, 0, nullptr) == 1 &&
          mdb_comoments_moments(nullptr, 0, 0, nullptr) == 0);

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
    const Bad bad[] = {{{0, 100, 4, INT64_MIN, INT64_MAX, 1, 1}, "which_mask must be 0 for mdb_comoments_buckets*."},
                       {{0, 0, 4, INT64_MIN, INT64_MAX, 1, 0}, "The bucket width must be positive."},
                       {{0, -7, 4, INT64_MIN, INT64_MAX, 1, 0}, "The bucket width must be positive."},
                       {{0, 100, 4, INT64_MIN, INT64_MAX, 0, 0}, "n_groups must be at least 1."},
                       {{0, 100, UINT64_MAX / 8, INT64_MIN, INT64_MAX, 4000000000u, 0}, "n_groups * n_buckets overflows."}};
    for (const Bad &b : bad) {
        CHECK(mdb_comoments_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &b.request, cells) == 1 && g_last_error == b.message);
        g_last_error.clear();
        CHECK(mdb_comoments_buckets(fake_context, &batch, &batch, nullptr, &b.request, cells) == 1 && g_last_error == b.message);
    }
    const mdb_bucket_request good = {0, 100, 4, INT64_MIN, INT64_MAX, 1, 0}, no_buckets = {0, 100, 0, INT64_MIN, INT64_MAX, 1, 0};
    CHECK(mdb_comoments_buckets_list(nullptr, inputs, 1, inputs, 1, nullptr, &good, cells) == 1 && g_last_error.find("NULL") != std::string::npos);
    CHECK(mdb_comoments_buckets_list(fake_context, nullptr, 1, inputs, 1, nullptr, &good, cells) == 1);
    CHECK(mdb_comoments_buckets_list(fake_context, inputs, 1, nullptr, 1, nullptr, &good, cells) == 1);
    CHECK(mdb_comoments_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, nullptr, cells) == 1);
    CHECK(mdb_comoments_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &good, nullptr) == 1);
    CHECK(mdb_comoments_buckets(fake_context, nullptr, &batch, nullptr, &good, cells) == 1);
    CHECK(mdb_comoments_buckets(fake_context, &batch, nullptr, nullptr, &good, cells) == 1 && g_last_error.find("y") != std::string::npos);
    CHECK(mdb_comoments_buckets_list(fake_context, with_null, 1, inputs, 1, nullptr, &good, cells) == 1 && g_last_error == "A batch of the list xs is NULL.");
    CHECK(mdb_comoments_buckets_list(fake_context, inputs, 1, with_null, 1, nullptr, &good, cells) == 1 && g_last_error == "A batch of the list ys is NULL.");
    CHECK(device_calls == 0);
    // nothing to do: success without the device
    batch.n = 0;
    CHECK(mdb_comoments_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &good, cells) == 0);
    CHECK(mdb_comoments_buckets_list(fake_context, inputs, 0, inputs, 0, nullptr, &good, cells) == 0);
    batch.n = 1;
    CHECK(mdb_comoments_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &no_buckets, cells) == 0 && device_calls == 0);
    CHECK(mdb_comoments_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &good, cells) == 0 && device_calls == 1);
    for (const mdb_comoments_cell &cell : cells) {
        mdb_comoments_cell untouched;
        std::memset(&untouched, 0xA5, sizeof untouched);
        CHECK(std::memcmp(&cell, &untouched, sizeof cell) == 0);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok: the host side of the covariance operator\n");
    return 0;
}
