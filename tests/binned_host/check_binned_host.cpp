// check_binned_host.cpp - TEST INFRASTRUCTURE: what mdb_binned_buckets* does before the device is needed
// (mdb_binned_host.cpp, mdb_binned.hpp), without a GPU. The arithmetic of the operator - pairs cut into runs where the
// value cell of x changes, every run summed around its first y value, the runs merged per cell - is driven with the
// functions the kernels use (moments_point, moments_finish, moments_merge, the cell rule of mdb_hist.hpp) and compared
// with long double sums over the same pairs; the host forms are handed malformed requests and edge lists: they must
// fail with their messages before binned_list_run - here a stand-in that counts its calls - is reached, and leave the
// cells alone.
#include "../../modelardb-rs_amd/csrc/mdb_binned.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

namespace mdb {
thread_local std::string g_last_error;
static int device_calls = 0;
int binned_list_run(mdb_ctx *, const mdb_segments *const *, uint32_t, const mdb_segments *const *, uint32_t,
                    const uint32_t *const *, const mdb_bucket_request *, const std::vector<int32_t> &, uint64_t,
                    mdb_moments_cell *) {
    device_calls++;
    return 0;
}
// (mdb_moments_host.cpp is linked for mdb_moments_merge_n: its own device step is not called here)
int moments_list_run(mdb_ctx *, const mdb_segments *const *, const uint32_t *const *, uint32_t, const mdb_bucket_request *,
                     uint64_t, mdb_moments_cell *) {
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

// The tolerances of tests/test_gpu_binned.py: 2^-44 of the largest |y| on the mean, 1e-5 of m2 on m2 (0: exactly 0).
static bool close_to(const mdb_moments_cell &cell, const Points &y) {
    if (cell.count != (int64_t)y.size()) return false;
    if (y.empty()) return cell.mean == 0.0 && cell.m2 == 0.0;
    long double sum = 0.0L, largest = 0.0L, m2 = 0.0L;
    for (float v : y) sum += (long double)v - (long double)y[0];
    const long double mean = (long double)y[0] + sum / (long double)y.size();
    for (float v : y) {
        m2 += ((long double)v - mean) * ((long double)v - mean);
        largest = std::fmax(largest, std::fabs((long double)v));
    }
    return std::fabs((long double)cell.mean - mean) <= std::ldexp(largest, -44) &&
           std::fabs((long double)cell.m2 - m2) <= 1e-5L * m2 && cell.m2 >= 0.0;
}

static mdb_moments_cell run_cell(const Points &y, size_t a, size_t b) {
    MomentsRun run = moments_run_empty();
    for (size_t k = a; k < b; k++) moments_point(run, y[k]);
    return moments_finish(run);
}

// The runs of the pairs (x, y): a new run where the cell of x changes, and after `longest` pairs (a bucket or segment
// boundary). Per cell the runs as cells, in order.
static std::vector<std::vector<mdb_moments_cell>> runs_per_cell(const Points &x, const Points &y,
                                                                const std::vector<int32_t> &edge_keys, size_t longest,
                                                                size_t *n_runs) {
    std::vector<std::vector<mdb_moments_cell>> runs(edge_keys.size() + 1);
    *n_runs = 0;
    size_t start = 0;
    for (size_t k = 1; k <= x.size(); k++) {
        const uint32_t cell = hist_cell_of_key(edge_keys, hist_key_of(x[start]));
        if (k == x.size() || k - start == longest || hist_cell_of_key(edge_keys, hist_key_of(x[k])) != cell) {
            runs[cell].push_back(run_cell(y, start, k));
            *n_runs += 1;
            start = k;
        }
    }
    return runs;
}

static mdb_moments_cell chain_of(const std::vector<mdb_moments_cell> &runs) {
    mdb_moments_cell chain = {0, 0.0, 0.0};
    for (const mdb_moments_cell &run : runs) CHECK(mdb_moments_merge_n(&chain, &run, 1) == 0);
    return chain;
}

// (the order of k_moments_tree: tiles of 64, each folded from its last entry backwards)
static mdb_moments_cell tree_of(std::vector<mdb_moments_cell> tiles) {
    if (tiles.empty()) return mdb_moments_cell{0, 0.0, 0.0};
    while (tiles.size() > 1) {
        std::vector<mdb_moments_cell> up;
        for (size_t a = 0; a < tiles.size(); a += 64) {
            const size_t b = std::min(tiles.size(), a + 64);
            mdb_moments_cell acc = tiles[b - 1];
            for (size_t t = b - 1; t > a; t--) moments_merge(acc, tiles[t - 1]);
            up.push_back(acc);
        }
        tiles = up;
    }
    return tiles[0];
}

int main() {
    std::mt19937_64 rng(20261019);
    std::normal_distribution<double> noise(0.0, 0.5);
    const float edge_values[3] = {9.7f, 10.0f, 10.3f};
    std::vector<int32_t> edge_keys;
    CHECK(hist_edge_keys(edge_values, 3, &edge_keys) == 0 && edge_keys.size() == 3);
    for (double level : {0.0, 1.0e6, 1.0e7}) {
        for (int constant = 0; constant < 2; constant++) {
            // x: noise around 10 that crosses the edges every few points; y: noise around the level, or one value
            Points x(20000), y(20000);
            for (size_t k = 0; k < x.size(); k++) {
                x[k] = (float)(10.0 + 0.6 * std::sin((double)k / 40.0) + 0.3 * noise(rng));
                y[k] = constant ? 1234.567f : (float)(level + noise(rng));
            }
            std::vector<Points> members(edge_keys.size() + 1);
            for (size_t k = 0; k < x.size(); k++) members[hist_cell_of_key(edge_keys, hist_key_of(x[k]))].push_back(y[k]);
            for (size_t longest : {(size_t)1, (size_t)7, (size_t)50, (size_t)745}) {
                size_t n_runs = 0;
                const std::vector<std::vector<mdb_moments_cell>> runs = runs_per_cell(x, y, edge_keys, longest, &n_runs);
                CHECK(n_runs >= x.size() / longest && n_runs <= x.size() && (longest == 1 || n_runs < x.size()));
                for (size_t c = 0; c < runs.size(); c++) {
                    CHECK(members[c].size() > 1000);
                    const mdb_moments_cell chain = chain_of(runs[c]), tree = tree_of(runs[c]);
                    CHECK(close_to(chain, members[c]) && close_to(tree, members[c]));
                    if (constant) // m2 is 0.0 and the mean the value exactly, in any order of merges
                        CHECK(chain.m2 == 0.0 && tree.m2 == 0.0 && chain.mean == (double)1234.567f && tree.mean == (double)1234.567f);
                }
            }
        }
    }
    // a non-finite y: the count is exact, neither mean nor m2 is finite - in its run and after merges on either side
    const float specials[] = {NAN, INFINITY, -INFINITY};
    for (float special : specials) {
        for (size_t position : {(size_t)0, (size_t)3, (size_t)9}) {
            Points y(10);
            for (float &v : y) v = (float)noise(rng);
            y[position] = special;
            const mdb_moments_cell one = run_cell(y, 0, y.size());
            CHECK(one.count == 10 && !std::isfinite(one.mean) && !std::isfinite(one.m2));
            Points other(5, 3.0f);
            mdb_moments_cell left = run_cell(other, 0, 5), right = one;
            const mdb_moments_cell finite = left;
            CHECK(mdb_moments_merge_n(&left, &one, 1) == 0 && mdb_moments_merge_n(&right, &finite, 1) == 0);
            CHECK(left.count == 15 && !std::isfinite(left.mean) && !std::isfinite(left.m2));
            CHECK(right.count == 15 && !std::isfinite(right.mean) && !std::isfinite(right.m2));
        }
    }
    // a non-finite x only decides the cell: the keys of NaN, +-0 and +-inf under the edges -inf, -0.0, +0.0, +inf
    const float wide[4] = {-INFINITY, -0.0f, 0.0f, INFINITY};
    std::vector<int32_t> wide_keys;
    CHECK(hist_edge_keys(wide, 4, &wide_keys) == 0);
    CHECK(hist_cell_of_key(wide_keys, hist_key_of(-NAN)) == 0 && hist_cell_of_key(wide_keys, hist_key_of(-INFINITY)) == 1);
    CHECK(hist_cell_of_key(wide_keys, hist_key_of(-1.0f)) == 1 && hist_cell_of_key(wide_keys, hist_key_of(-0.0f)) == 2);
    CHECK(hist_cell_of_key(wide_keys, hist_key_of(0.0f)) == 3 && hist_cell_of_key(wide_keys, hist_key_of(INFINITY)) == 4);
    CHECK(hist_cell_of_key(wide_keys, hist_key_of(NAN)) == 4);

    // the host forms: malformed requests and edge lists fail before the device step
    mdb_ctx *fake_context = reinterpret_cast<mdb_ctx *>(8); // (never dereferenced)
    mdb_segments batch;
    std::memset(&batch, 0, sizeof batch);
    batch.n = 1;
    const mdb_segments *inputs[1] = {&batch};
    const mdb_segments *with_null[1] = {nullptr};
    mdb_moments_cell cells[16];
    std::memset(cells, 0xA5, sizeof cells);
    struct Bad {
        mdb_bucket_request request;
        const char *message;
    };
    const Bad bad[] = {{{0, 100, 4, INT64_MIN, INT64_MAX, 1, 1}, "which_mask must be 0 for mdb_binned_buckets*."},
                       {{0, 0, 4, INT64_MIN, INT64_MAX, 1, 0}, "The bucket width must be positive."},
                       {{0, -7, 4, INT64_MIN, INT64_MAX, 1, 0}, "The bucket width must be positive."},
                       {{0, 100, 4, INT64_MIN, INT64_MAX, 0, 0}, "n_groups must be at least 1."},
                       {{0, 100, UINT64_MAX / 8, INT64_MIN, INT64_MAX, 4000000000u, 0}, "n_groups * n_buckets * n_cells overflows."},
                       {{0, 100, UINT64_MAX / 64, INT64_MIN, INT64_MAX, 1, 0}, "n_groups * n_buckets * n_cells overflows."}};
    for (const Bad &b : bad) {
        CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &b.request, edge_values, 3, cells) == 1 && g_last_error == b.message);
        g_last_error.clear();
        CHECK(mdb_binned_buckets(fake_context, &batch, &batch, nullptr, &b.request, edge_values, 3, cells) == 1 && g_last_error == b.message);
    }
    const mdb_bucket_request good = {0, 100, 4, INT64_MIN, INT64_MAX, 1, 0}, no_buckets = {0, 100, 0, INT64_MIN, INT64_MAX, 1, 0};
    const float equal[2] = {1.0f, 1.0f}, descending[2] = {2.0f, 1.0f}, zeros[2] = {0.0f, -0.0f}, nans[2] = {NAN, NAN};
    for (const float *edges : {equal, descending, zeros, nans}) {
        CHECK(mdb_binned_buckets(fake_context, &batch, &batch, nullptr, &good, edges, 2, cells) == 1 &&
              g_last_error.find("strictly increasing in totalOrder") != std::string::npos);
    }
    const float ordered_zeros[2] = {-0.0f, 0.0f};
    std::vector<int32_t> keys;
    uint64_t n_cells = 0;
    CHECK(binned_arguments_check(&good, ordered_zeros, 2, &keys, &n_cells) == 0 && n_cells == 12 && keys.size() == 2);
    std::vector<float> many(MDB_HIST_MAX_EDGES + 1);
    for (size_t k = 0; k < many.size(); k++) many[k] = (float)k;
    CHECK(mdb_binned_buckets(fake_context, &batch, &batch, nullptr, &good, many.data(), 0, cells) == 1 && g_last_error.find("n_edges") != std::string::npos);
    CHECK(mdb_binned_buckets(fake_context, &batch, &batch, nullptr, &good, many.data(), MDB_HIST_MAX_EDGES + 1, cells) == 1 &&
          g_last_error.find("n_edges") != std::string::npos);
    CHECK(binned_arguments_check(&good, many.data(), MDB_HIST_MAX_EDGES, &keys, &n_cells) == 0 && n_cells == 4ull * (MDB_HIST_MAX_EDGES + 1));
    CHECK(mdb_binned_buckets_list(nullptr, inputs, 1, inputs, 1, nullptr, &good, edge_values, 3, cells) == 1 && g_last_error.find("NULL") != std::string::npos);
    CHECK(mdb_binned_buckets_list(fake_context, nullptr, 1, inputs, 1, nullptr, &good, edge_values, 3, cells) == 1);
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, nullptr, 1, nullptr, &good, edge_values, 3, cells) == 1);
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, nullptr, edge_values, 3, cells) == 1);
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &good, nullptr, 3, cells) == 1);
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &good, edge_values, 3, nullptr) == 1);
    CHECK(mdb_binned_buckets(fake_context, nullptr, &batch, nullptr, &good, edge_values, 3, cells) == 1);
    CHECK(mdb_binned_buckets(fake_context, &batch, nullptr, nullptr, &good, edge_values, 3, cells) == 1 && g_last_error.find("y") != std::string::npos);
    CHECK(mdb_binned_buckets_list(fake_context, with_null, 1, inputs, 1, nullptr, &good, edge_values, 3, cells) == 1 && g_last_error == "A batch of the list xs is NULL.");
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, with_null, 1, nullptr, &good, edge_values, 3, cells) == 1 && g_last_error == "A batch of the list ys is NULL.");
    CHECK(device_calls == 0);
    // nothing to do: success without the device
    batch.n = 0;
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &good, edge_values, 3, cells) == 0);
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 0, inputs, 0, nullptr, &good, edge_values, 3, cells) == 0);
    batch.n = 1;
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &no_buckets, edge_values, 3, cells) == 0 && device_calls == 0);
    CHECK(mdb_binned_buckets_list(fake_context, inputs, 1, inputs, 1, nullptr, &good, edge_values, 3, cells) == 0 && device_calls == 1);
    for (const mdb_moments_cell &cell : cells) {
        mdb_moments_cell untouched;
        std::memset(&untouched, 0xA5, sizeof untouched);
        CHECK(std::memcmp(&cell, &untouched, sizeof cell) == 0);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok: the host side of the binned moments\n");
    return 0;
}
