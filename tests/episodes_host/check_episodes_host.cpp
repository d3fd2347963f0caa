// TEST INFRASTRUCTURE: the run monoid and the attribution rule of the episode operator
// (modelardb-rs_amd/csrc/mdb_episodes.hpp, the text the kernels compile) checked on the host against a direct
// row-by-row loop. For a few thousand seeded random row arrays - pass bits, timestamps with equal and backwards
// steps, groups, values with NaN and +-0 - the rows are cut into random segments (zero-row ones included), every
// segment is summarised, the summaries are folded left to right and in random bracketings, and the episodes the
// attribution rule emits from the exclusive folds are compared with the loop's: every field but `sum` exactly, `sum`
// exactly where the values are small integers. Associativity of everything but `sum` is part of the check.
// Prints "ok: ..." or lines with MISMATCH and exits 1.
#include "../../modelardb-rs_amd/csrc/mdb_episodes.hpp"

#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace mdb;

namespace {

struct Row {
    int64_t t;
    float v;
    uint32_t group;
    uint32_t segment;
    bool pass;
};

int failures = 0;

void mismatch(const char *what, uint64_t trial) {
    if (failures++ < 20) std::printf("MISMATCH %s in trial %" PRIu64 "\n", what, trial);
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// Every field; the sum only if `with_sum`.
bool same_episode(const mdb_episode &a, const mdb_episode &b, bool with_sum) {
    return a.first_row == b.first_row && a.count == b.count && a.t_first == b.t_first && a.t_last == b.t_last &&
           same_bits(a.min, b.min) && same_bits(a.max, b.max) && a.group == b.group && a.first_segment == b.first_segment &&
           a.reserved == b.reserved && (!with_sum || std::memcmp(&a.sum, &b.sum, 8) == 0);
}
bool same_run(const mdb_episode &a, const mdb_episode &b, bool with_sum) {
    if (a.count == 0 || b.count == 0) return a.count == b.count;
    return same_episode(a, b, with_sum);
}
bool same_summary(const EpisodeSummary &a, const EpisodeSummary &b, bool with_sum) {
    if (a.rows == 0 || b.rows == 0) return a.rows == b.rows;
    return a.rows == b.rows && a.t_front == b.t_front && a.t_back == b.t_back && a.g_front == b.g_front &&
           a.g_back == b.g_back && a.whole == b.whole && a.closed == b.closed && a.passing == b.passing &&
           same_run(a.head, b.head, with_sum) && same_run(a.tail, b.tail, with_sum);
}

// The definition: one loop over the rows.
std::vector<mdb_episode> direct(const std::vector<Row> &rows, const EpisodeRule &rule, bool filtered) {
    std::vector<mdb_episode> out;
    mdb_episode open = episode_none();
    auto close = [&]() {
        if (open.count != 0 && (!filtered || episode_reported(rule, open))) out.push_back(open);
        open = episode_none();
    };
    for (size_t r = 0; r < rows.size(); r++) {
        const Row &row = rows[r];
        const bool goes_on = r > 0 && episode_continues(rule, rows[r - 1].t, rows[r - 1].group, row.t, row.group);
        if (!row.pass) {
            close();
            continue;
        }
        if (open.count != 0 && !goes_on) close();
        if (open.count == 0) {
            open = episode_of_row(r, row.segment, row.group, row.t, row.v);
        } else {
            open.count += 1;
            open.t_last = row.t;
            open.sum += (double)row.v;
            open.min = episode_min(open.min, row.v);
            open.max = episode_max(open.max, row.v);
        }
    }
    close();
    return out;
}

// The summary of rows [a, b) (one segment), and the reported runs strictly inside it.
EpisodeSummary summarise(const std::vector<Row> &rows, size_t a, size_t b, const EpisodeRule &rule,
                         std::vector<mdb_episode> *inside) {
    EpisodeSummary s = episode_summary_none();
    if (a == b) return s;
    s.rows = b - a;
    s.t_front = rows[a].t;
    s.t_back = rows[b - 1].t;
    s.g_front = rows[a].group;
    s.g_back = rows[b - 1].group;
    const std::vector<Row> part(rows.begin() + a, rows.begin() + b);
    std::vector<mdb_episode> runs = direct(part, rule, false);
    for (mdb_episode &run : runs) {
        run.first_row += a;
        s.passing += run.count;
        const bool is_head = run.first_row == a, is_tail = run.first_row + run.count == b;
        if (is_head) s.head = run;
        if (is_tail) s.tail = run;
        if (is_head && is_tail) s.whole = 1;
        if (!is_head && !is_tail && episode_reported(rule, run)) {
            s.closed += 1;
            inside->push_back(run);
        }
    }
    return s;
}

// The fold of summaries [a, b) in a random bracketing.
EpisodeSummary fold_random(const std::vector<EpisodeSummary> &s, size_t a, size_t b, const EpisodeRule &rule, std::mt19937_64 &rng) {
    if (a == b) return episode_summary_none();
    if (b - a == 1) return s[a];
    const size_t cut = a + 1 + rng() % (b - a - 1);
    const EpisodeSummary left = fold_random(s, a, cut, rule, rng), right = fold_random(s, cut, b, rule, rng);
    return episode_combine(rule, left, right);
}

void trial(uint64_t seed) {
    std::mt19937_64 rng(seed);
    const size_t n = rng() % 200;
    const bool integers = rng() % 2 == 0; // small integers: every f64 sum is exact in any grouping
    static const uint32_t PASS_PERCENT[4] = {5, 50, 90, 100};
    const uint32_t pass_percent = PASS_PERCENT[rng() % 4];
    std::vector<Row> rows(n);
    int64_t t = (int64_t)(rng() % 3 == 0 ? std::numeric_limits<int64_t>::min() + 10000 + (int64_t)(rng() % 50) : (int64_t)(rng() % 1000));
    uint32_t group = 0;
    for (size_t r = 0; r < n; r++) {
        const uint32_t step = rng() % 16;
        if (step == 0) t -= (int64_t)(rng() % 40);          // backwards
        else if (step >= 3) t += (int64_t)(rng() % 12) + 1; // (1, 2: equal timestamps)
        if (rng() % 40 == 0) group = (uint32_t)(rng() % 3);
        float v = integers ? (float)((int)(rng() % 9) - 4) : (float)((double)(rng() % 100000) / 7.0 - 5000.0);
        const uint32_t special = rng() % 30;
        if (!integers && special == 0) v = std::numeric_limits<float>::quiet_NaN();
        if (special == 1) v = -0.0f;
        if (special == 2) v = 0.0f;
        rows[r] = Row{t, v, group, 0, rng() % 100 < pass_percent};
    }
    EpisodeRule rule;
    static const int64_t MAX_GAP[5] = {0, 1, 5, 11, std::numeric_limits<int64_t>::max()};
    static const int64_t MIN_DURATION[4] = {0, 0, 3, 20};
    static const uint64_t MIN_COUNT[4] = {0, 1, 2, 5};
    rule.max_gap = MAX_GAP[rng() % 5];
    rule.min_duration = MIN_DURATION[rng() % 4];
    rule.min_count = MIN_COUNT[rng() % 4];
    // the cut into segments, zero-row ones included
    std::vector<size_t> bounds{0};
    while (bounds.back() < n) {
        const uint32_t kind = rng() % 8;
        const size_t length = kind == 0 ? 0 : (kind < 5 ? 1 + rng() % 3 : 1 + rng() % 40);
        bounds.push_back(std::min(n, bounds.back() + length));
    }
    for (uint32_t k = rng() % 3; k > 0; k--) bounds.push_back(n); // zero-row segments behind the last row
    const size_t n_segments = bounds.size() - 1;
    for (size_t i = 0; i < n_segments; i++)
        for (size_t r = bounds[i]; r < bounds[i + 1]; r++) rows[r].segment = (uint32_t)i;

    const std::vector<mdb_episode> expected = direct(rows, rule, true);
    std::vector<EpisodeSummary> summaries(n_segments);
    std::vector<std::vector<mdb_episode>> inside(n_segments);
    for (size_t i = 0; i < n_segments; i++) summaries[i] = summarise(rows, bounds[i], bounds[i + 1], rule, &inside[i]);
    size_t last_with_rows = n_segments;
    for (size_t i = 0; i < n_segments; i++)
        if (summaries[i].rows != 0) last_with_rows = i;

    for (int bracketing = 0; bracketing < 3; bracketing++) {
        std::vector<mdb_episode> emitted;
        EpisodeSummary running = episode_summary_none();
        for (size_t i = 0; i < n_segments; i++) {
            // the exclusive fold in front of segment i: left to right, or a random tree
            const EpisodeSummary before = bracketing == 0 ? running : fold_random(summaries, 0, i, rule, rng);
            if (!same_summary(before, running, integers)) mismatch("associativity of the fold", seed);
            const EpisodeEnds ends = episode_attribute(rule, episode_prefix_of(before), summaries[i], i == last_with_rows);
            if (ends.emit_incoming) emitted.push_back(ends.incoming);
            if (ends.emit_first) emitted.push_back(ends.first);
            emitted.insert(emitted.end(), inside[i].begin(), inside[i].end());
            if (ends.emit_open) emitted.push_back(ends.open);
            running = episode_combine(rule, running, summaries[i]);
        }
        if (emitted.size() != expected.size()) {
            mismatch("number of episodes", seed);
            continue;
        }
        for (size_t k = 0; k < expected.size(); k++) {
            if (!same_episode(emitted[k], expected[k], integers)) mismatch("episode", seed);
            if (!integers && !(emitted[k].sum == expected[k].sum || (emitted[k].sum != emitted[k].sum && expected[k].sum != expected[k].sum) ||
                               std::fabs(emitted[k].sum - expected[k].sum) <= 1e-9 * 5000.0 * (double)expected[k].count))
                mismatch("sum beyond rounding", seed);
        }
        // the fold of everything counts the episodes too
        const uint64_t counted = running.closed + (episode_reported(rule, running.head) ? 1 : 0) +
                                 (!running.whole && episode_reported(rule, running.tail) ? 1 : 0);
        if (counted != expected.size()) mismatch("episodes counted by the fold", seed);
        uint64_t passing = 0;
        for (const Row &row : rows) passing += row.pass ? 1 : 0;
        if (running.passing != passing) mismatch("passing rows", seed);
    }
}

} // namespace

int main() {
    static_assert(sizeof(mdb_episode) == 64 && sizeof(mdb_episodes_request) == 64, "the layout of the header");
    const uint64_t trials = 4000;
    for (uint64_t seed = 1; seed <= trials; seed++) trial(seed);
    if (failures) {
        std::printf("%d MISMATCH lines\n", failures);
        return 1;
    }
    std::printf("ok: %" PRIu64 " random row arrays, left-to-right and random bracketings\n", trials);
    return 0;
}
