// mdb_episodes.hpp - the arithmetic of the episode operator (mdb_episodes*, mdb_episodes.hip) that needs no device:
// when a row continues its predecessor, how two runs join, the SUMMARY of a stretch of consecutive rows, the monoid
// that stitches the summaries of neighbouring stretches, and the attribution rule that says which episodes a stretch
// emits once it knows what reaches it from the left. Plain __host__ __device__ code without a HIP type: the kernels
// and the check program tests/episodes_host (g++, CPU sanitizers) compile the same text.
//
//   run        a maximal set of consecutive passing rows, each but the first continuing its predecessor: an
//              mdb_episode (count == 0: no run).
//   summary    of a stretch of rows (a segment, or several segments in a row): its number of rows, timestamp and
//              group of its first and last row, the HEAD run (begins at the stretch's first row), the TAIL run (ends
//              at its last row), whether one run covers every row (then head == tail), the number of reported runs
//              that begin after the first row and end before the last one, and the passing rows.
//   A (+) B    A's tail is joined to B's head iff both exist and B's first row continues A's last row. What was
//              open at the seam and is not joined closes there. A stretch without rows is the identity. Everything
//              but the f64 `sum` of a joined run is associative exactly; `sum` is associative up to rounding.
//   attribute  a stretch S with the fold P of everything to its left emits, in this order: P's tail if S's first row
//              does not continue it; S's head - joined with P's tail if it does - unless it covers all of S; the runs
//              strictly inside S; and, only if S is the last stretch with rows, whatever is still open at its end.
//              So no stretch looks ahead: a run is emitted by the stretch that sees it end.
#pragma once

#include "../../include/mdb.h"

#include <cfloat>
#include <cstdint>

#if defined(__HIPCC__)
#define MDB_EP_FN __host__ __device__ __forceinline__
#else
#define MDB_EP_FN inline
#endif

namespace mdb {

struct EpisodeRule {
    int64_t max_gap;
    int64_t min_duration;
    uint64_t min_count;
};

// Does a row (t, g) continue its predecessor (t_prev, g_prev)? The difference is formed after the comparison, in
// uint64_t: it cannot overflow.
MDB_EP_FN bool episode_continues(const EpisodeRule &rule, int64_t t_prev, uint32_t g_prev, int64_t t, uint32_t g) {
    return g == g_prev && t >= t_prev && (uint64_t)t - (uint64_t)t_prev <= (uint64_t)rule.max_gap;
}

// fmin / fmax as mdb_agg_state folds them: a NaN is skipped, the first operand kept on ties.
MDB_EP_FN float episode_min(float a, float b) {
    if (a != a) return b;
    return (b < a) ? b : a;
}
MDB_EP_FN float episode_max(float a, float b) {
    if (a != a) return b;
    return (b > a) ? b : a;
}

MDB_EP_FN mdb_episode episode_none() {
    mdb_episode e;
    e.first_row = 0;
    e.count = 0;
    e.t_first = 0;
    e.t_last = 0;
    e.sum = 0.0;
    e.min = FLT_MAX;
    e.max = -FLT_MAX;
    e.group = 0;
    e.first_segment = 0;
    e.reserved = 0;
    return e;
}

// The run of one row.
MDB_EP_FN mdb_episode episode_of_row(uint64_t row, uint32_t segment, uint32_t group, int64_t t, float v) {
    mdb_episode e = episode_none();
    e.first_row = row;
    e.count = 1;
    e.t_first = t;
    e.t_last = t;
    e.sum = (double)v;
    e.min = episode_min(e.min, v);
    e.max = episode_max(e.max, v);
    e.group = group;
    e.first_segment = segment;
    return e;
}

// a, then b right behind it (either may be no run).
MDB_EP_FN mdb_episode episode_join(const mdb_episode &a, const mdb_episode &b) {
    if (a.count == 0) return b;
    if (b.count == 0) return a;
    mdb_episode e = a;
    e.count = a.count + b.count;
    e.t_last = b.t_last;
    e.sum = a.sum + b.sum;
    e.min = episode_min(a.min, b.min);
    e.max = episode_max(a.max, b.max);
    return e;
}

// The minimum filters. (t_last >= t_first inside a run: every step is a non-negative one)
MDB_EP_FN bool episode_reported(const EpisodeRule &rule, const mdb_episode &e) {
    return e.count != 0 && e.count >= rule.min_count &&
           (uint64_t)e.t_last - (uint64_t)e.t_first >= (uint64_t)rule.min_duration;
}

struct EpisodeSummary {
    uint64_t rows; // 0: the identity
    int64_t t_front, t_back;
    uint32_t g_front, g_back;
    uint32_t whole; // one run covers every row
    uint32_t pad;
    uint64_t closed;  // reported runs strictly inside
    uint64_t passing; // passing rows
    mdb_episode head, tail;
};

MDB_EP_FN EpisodeSummary episode_summary_none() {
    EpisodeSummary s;
    s.rows = 0;
    s.t_front = s.t_back = 0;
    s.g_front = s.g_back = 0;
    s.whole = 0;
    s.pad = 0;
    s.closed = 0;
    s.passing = 0;
    s.head = episode_none();
    s.tail = episode_none();
    return s;
}

// The monoid.
MDB_EP_FN EpisodeSummary episode_combine(const EpisodeRule &rule, const EpisodeSummary &a, const EpisodeSummary &b) {
    if (a.rows == 0) return b;
    if (b.rows == 0) return a;
    EpisodeSummary r;
    r.rows = a.rows + b.rows;
    r.t_front = a.t_front;
    r.g_front = a.g_front;
    r.t_back = b.t_back;
    r.g_back = b.g_back;
    r.whole = 0;
    r.pad = 0;
    r.closed = a.closed + b.closed;
    r.passing = a.passing + b.passing;
    r.head = a.head;
    r.tail = b.tail;
    const bool joined = a.tail.count != 0 && b.head.count != 0 &&
                        episode_continues(rule, a.t_back, a.g_back, b.t_front, b.g_front);
    if (joined) {
        const mdb_episode both = episode_join(a.tail, b.head);
        if (a.whole) r.head = both;
        if (b.whole) r.tail = both;
        if (a.whole && b.whole) r.whole = 1;
        if (!a.whole && !b.whole && episode_reported(rule, both)) r.closed += 1;
    } else {
        // (a run that covers all of a is r's head, one that covers all of b r's tail: neither is inside)
        if (!a.whole && episode_reported(rule, a.tail)) r.closed += 1;
        if (!b.whole && episode_reported(rule, b.head)) r.closed += 1;
    }
    return r;
}

// What a stretch needs of the fold of everything to its left.
struct EpisodePrefix {
    mdb_episode tail; // the open run that reaches the stretch (count == 0: none)
    int64_t t_back;
    uint32_t g_back;
    uint32_t rows; // 0: nothing to the left has rows
};

MDB_EP_FN EpisodePrefix episode_prefix_of(const EpisodeSummary &s) {
    EpisodePrefix p;
    p.tail = s.rows != 0 ? s.tail : episode_none();
    p.t_back = s.t_back;
    p.g_back = s.g_back;
    p.rows = s.rows != 0 ? 1u : 0u;
    return p;
}

// The attribution rule: what stretch s emits apart from its inside runs. In front of them: `incoming` (the run that
// reaches s and ends in front of it) if emit_incoming, then `first` (s's head, with what it continues) if emit_first;
// behind them: `open` if emit_open. last: s is the last stretch with rows.
struct EpisodeEnds {
    mdb_episode incoming, first, open;
    uint32_t emit_incoming, emit_first, emit_open;
    MDB_EP_FN uint32_t before() const { return emit_incoming + emit_first; }
};

MDB_EP_FN EpisodeEnds episode_attribute(const EpisodeRule &rule, const EpisodePrefix &p, const EpisodeSummary &s, bool last) {
    EpisodeEnds e;
    e.emit_incoming = e.emit_first = e.emit_open = 0;
    e.incoming = e.first = e.open = episode_none();
    if (s.rows == 0) return e;
    const bool reaches = p.rows != 0 && p.tail.count != 0;
    const bool joined = reaches && s.head.count != 0 && episode_continues(rule, p.t_back, p.g_back, s.t_front, s.g_front);
    if (reaches && !joined) {
        e.incoming = p.tail;
        e.emit_incoming = episode_reported(rule, p.tail) ? 1u : 0u;
    }
    e.first = joined ? episode_join(p.tail, s.head) : s.head;
    if (s.whole) {
        e.open = e.first;
    } else {
        e.emit_first = episode_reported(rule, e.first) ? 1u : 0u;
        e.open = s.tail;
    }
    e.emit_open = last && episode_reported(rule, e.open) ? 1u : 0u;
    return e;
}

} // namespace mdb
