// check_hist_buckets_host.cpp - TEST INFRASTRUCTURE: the selection step of mdb_quantile_buckets* (mdb_select.hpp) without
// a GPU. A pass of the counting kernel is made here from plain arrays: per (cell, rank) the points of the cell whose
// unsigned key carries the rank's prefix, counted by the next digit - what WindowLane::flush adds - and the step that
// k_quantile_select runs per (cell, rank) is run on those counts. After SELECT_PASSES passes every order statistic of
// every cell must have the bits of the sorted cell's. Built plain and with -fsanitize=address,undefined
// (tests/test_hist_buckets_cpu.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mdb_hist.hpp"
#include "mdb_select.hpp"

namespace mdb {
thread_local std::string g_last_error; // (the library's own lives in mdb_ctx.hip)
} // namespace mdb

using namespace mdb;

static int mismatches = 0;
static void expect(bool ok, const char *what, uint64_t a = 0, uint64_t b = 0) {
    if (ok) return;
    mismatches++;
    if (mismatches < 20) std::printf("MISMATCH %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
}

// The order statistics of every cell for the quantiles q, by the passes of the selection: keys[c] are the totalOrder keys
// of cell c in any order. out[c][rank]: the selected key (untouched for an empty cell).
static void select_all(const std::vector<std::vector<int32_t>> &keys, const std::vector<double> &q,
                       std::vector<std::vector<int32_t>> *out, std::vector<uint64_t> *n_points) {
    const uint32_t n_ranks = 2 * (uint32_t)q.size();
    const size_t n_cells = keys.size();
    std::vector<uint32_t> prefixes(n_cells * n_ranks, 0);
    std::vector<uint64_t> remaining(n_cells * n_ranks, 0);
    n_points->assign(n_cells, 0);
    for (uint32_t pass = 0; pass < SELECT_PASSES; pass++) {
        const uint32_t pass_ranks = pass == 0 ? 1u : n_ranks, shift = select_shift(pass);
        std::vector<uint64_t> windows(n_cells * pass_ranks * SELECT_DIGITS, 0);
        for (size_t c = 0; c < n_cells; c++)
            for (int32_t key : keys[c]) { // the counting pass: WindowLane, one point at a time
                const uint32_t cell = select_ukey(key) >> shift;
                const uint32_t digit = cell & (SELECT_DIGITS - 1), above = cell >> SELECT_DIGIT_BITS;
                for (uint32_t rank = 0; rank < pass_ranks; rank++)
                    if (pass == 0 || prefixes[c * n_ranks + rank] == above)
                        windows[(c * pass_ranks + rank) * SELECT_DIGITS + digit] += 1;
            }
        for (size_t lane = 0; lane < n_cells * n_ranks; lane++) { // the selection: k_quantile_select
            const size_t c = lane / n_ranks;
            const uint32_t rank = (uint32_t)(lane % n_ranks);
            const uint64_t *window = windows.data() + (pass == 0 ? c : lane) * SELECT_DIGITS;
            uint64_t wanted;
            if (pass == 0) {
                uint64_t n = 0;
                for (uint32_t digit = 0; digit < SELECT_DIGITS; digit++) n += window[digit];
                (*n_points)[c] = n;
                if (n == 0) continue;
                uint64_t rank_lo, rank_hi;
                select_ranks(q[rank / 2], n, &rank_lo, &rank_hi);
                wanted = rank % 2 ? rank_hi : rank_lo;
            } else {
                if ((*n_points)[c] == 0) continue;
                wanted = remaining[lane];
            }
            uint64_t in_window = 0;
            for (uint32_t digit = 0; digit < SELECT_DIGITS; digit++) in_window += window[digit];
            expect(wanted < in_window, "the rank lies inside its window", wanted, in_window);
            uint64_t left = 0;
            const uint32_t digit = select_digit(window, SELECT_DIGITS, wanted, &left);
            expect(digit < SELECT_DIGITS && left < window[digit], "the remaining rank lies inside the digit", left, digit);
            prefixes[lane] = (prefixes[lane] << SELECT_DIGIT_BITS) | digit;
            remaining[lane] = left;
        }
    }
    out->assign(n_cells, std::vector<int32_t>(n_ranks, 0));
    for (size_t c = 0; c < n_cells; c++)
        for (uint32_t rank = 0; rank < n_ranks; rank++) {
            (*out)[c][rank] = select_key_of_ukey(prefixes[c * n_ranks + rank]);
            if ((*n_points)[c]) expect(remaining[c * n_ranks + rank] < keys[c].size(), "a rank remains below the cell's size");
        }
}

int main() {
    std::mt19937_64 rng(2040);
    const uint32_t specials[] = {0x00000000u, 0x80000000u, 0x7fc00000u, 0xffc00000u, 0x7f800000u, 0xff800000u,
                                 0x7fffffffu, 0xffffffffu, 0x00000001u, 0x80000001u, 0x3f800000u, 0xbf800000u};
    // (cell, key) samples: cells of 0, 1, 2, 3 points, small cells of specials, cells of few distinct values (ranks
    // that cross a run of equal keys), wide random cells, cells inside one digit of the top pass.
    std::vector<std::vector<int32_t>> keys;
    keys.push_back({});
    for (uint32_t bits : specials) keys.push_back({hist_key_of_bits(bits)});
    for (int c = 0; c < 200; c++) {
        std::vector<int32_t> cell;
        const int kind = c % 5;
        const size_t n = kind == 0 ? (size_t)(rng() % 4) : (size_t)(1 + rng() % 700);
        const uint32_t base = (uint32_t)rng();
        for (size_t k = 0; k < n; k++) {
            uint32_t bits;
            if (kind == 1) bits = specials[rng() % 12];
            else if (kind == 2) bits = base + (uint32_t)(rng() % 3);            // three distinct keys, long runs
            else if (kind == 3) bits = (base & 0xffffff00u) | (uint32_t)(rng() & 0xffu); // one window until the last pass
            else bits = (uint32_t)rng();
            cell.push_back(hist_key_of_bits(bits));
        }
        keys.push_back(cell);
    }
    keys.push_back({});
    const std::vector<std::vector<double>> quantiles = {{0.5}, {0.0, 0.25, 0.5, 1.0}, {0.999}, {0.5, 0.95, 0.99}};
    uint64_t checked = 0, empty = 0, single = 0;
    for (const std::vector<double> &q : quantiles) {
        std::vector<std::vector<int32_t>> got;
        std::vector<uint64_t> n_points;
        select_all(keys, q, &got, &n_points);
        for (size_t c = 0; c < keys.size(); c++) {
            std::vector<int32_t> sorted = keys[c];
            std::sort(sorted.begin(), sorted.end());
            expect(n_points[c] == sorted.size(), "n_points", n_points[c], sorted.size());
            if (sorted.empty()) {
                empty++;
                continue;
            }
            single += sorted.size() == 1;
            for (size_t i = 0; i < q.size(); i++) {
                uint64_t rank_lo, rank_hi, lo2, hi2;
                double fraction;
                if (quantile_ranks(q[i], sorted.size(), &rank_lo, &rank_hi, &fraction)) return 2;
                select_ranks(q[i], sorted.size(), &lo2, &hi2);
                expect(rank_lo == lo2 && rank_hi == hi2, "select_ranks is quantile_ranks", lo2, rank_lo);
                // (bits, not values: NaNs and signed zeros are points like any other)
                expect(hist_bits_of_key(got[c][2 * i]) == hist_bits_of_key(sorted[rank_lo]), "lo", c, i);
                expect(hist_bits_of_key(got[c][2 * i + 1]) == hist_bits_of_key(sorted[rank_hi]), "hi", c, i);
                checked += 2;
            }
        }
    }
    // EVERY order statistic of EVERY cell: q = r / (N - 1) is not exact in f64 for each rank r, so the ranks are driven
    // directly - the step alone, pass by pass, on one cell at a time.
    for (size_t c = 0; c < keys.size(); c++) {
        std::vector<int32_t> sorted = keys[c];
        std::sort(sorted.begin(), sorted.end());
        for (uint64_t rank = 0; rank < sorted.size(); rank++) {
            uint32_t prefix = 0;
            uint64_t wanted = rank;
            for (uint32_t pass = 0; pass < SELECT_PASSES; pass++) {
                uint64_t window[SELECT_DIGITS] = {};
                const uint32_t shift = select_shift(pass);
                for (int32_t key : keys[c]) {
                    const uint32_t cell = select_ukey(key) >> shift;
                    if (pass == 0 || (cell >> SELECT_DIGIT_BITS) == prefix) window[cell & (SELECT_DIGITS - 1)] += 1;
                }
                prefix = (prefix << SELECT_DIGIT_BITS) | select_digit(window, SELECT_DIGITS, wanted, &wanted);
            }
            expect(select_key_of_ukey(prefix) == sorted[rank], "every rank of a cell", c, rank);
            checked++;
        }
    }
    // The edges of the ranks: N = 1, the last rank, N beyond 2^53.
    uint64_t lo = 9, hi = 9;
    select_ranks(1.0, 1, &lo, &hi);
    expect(lo == 0 && hi == 0, "one point");
    select_ranks(1.0, UINT64_MAX, &lo, &hi);
    expect(lo == UINT64_MAX - 1 && hi == UINT64_MAX - 1, "no rank past the last point", lo, hi);
    select_ranks(0.5, 4, &lo, &hi);
    expect(lo == 1 && hi == 2, "an even count", lo, hi);
    // Counts above 2^32 in a digit.
    {
        uint64_t window[SELECT_DIGITS] = {};
        window[3] = 5'000'000'000ull;
        window[200] = 7'000'000'000ull;
        uint64_t left = 0;
        expect(select_digit(window, SELECT_DIGITS, 4'999'999'999ull, &left) == 3 && left == 4'999'999'999ull, "below 2^33");
        expect(select_digit(window, SELECT_DIGITS, 5'000'000'000ull, &left) == 200 && left == 0, "the first of the next digit");
        expect(select_digit(window, SELECT_DIGITS, 11'999'999'999ull, &left) == 200 && left == 6'999'999'999ull, "the last point");
    }
    expect(empty >= 8 && single >= 40, "empty and one-point cells occur", empty, single);
    if (mismatches) {
        std::printf("FAILED: %d mismatches\n", mismatches);
        return 1;
    }
    std::printf("ok: %llu order statistics of %zu cells (%llu empty, %llu of one point)\n", (unsigned long long)checked,
                keys.size(), (unsigned long long)empty, (unsigned long long)single);
    return 0;
}
