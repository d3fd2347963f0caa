// mdb_episodes.hip - episodes on segments: the maximal runs of rows that pass a value predicate, each row continuing
// its predecessor (mdb_episodes, mdb_episodes_list, mdb_episodes_dev, mdb_episodes_count_dev; the contract: mdb.h).
//
// What the reference computes with GridExec -> FilterExec -> WindowAggExec (lag) -> AggregateExec over every rebuilt
// point. Here a segment becomes a SUMMARY (mdb_episodes.hpp), the summaries are stitched by a device-wide scan under
// the run monoid, and every run is emitted by the segment that sees it end - so no segment looks ahead, and an
// episode that spans thousands of segments costs what any other does.
//
//   rows and first rows     the range grid's prepass (grid_range_plan: every error the range calls report) and an
//                           exclusive scan (mdb_scan.hpp), as the masks do: the row numbering is theirs.
//   k_episodes_classify     1 lane / segment: the group id checked (every segment, inside the range or not), then
//                           PMC-Mean / Swing on regular timestamps whose interval steps within max_gap: the passing
//                           model points are one interval (model_run, mdb_filter.hpp), its aggregate the closed form
//                           of the filtered aggregates (model_closed_form) - the summary in O(1) / O(log n). Everything
//                           else is marked per point: MacaqueV, irregular timestamps, residual tails, a Swing end
//                           that evaluates to NaN, a sampling interval beyond max_gap.
//   k_episodes_points       the per-point segments: gathered and rebuilt by the range grid in bounded slices
//                           (filter_tested_slices, mdb_filter_points.hpp), WITH their timestamps, then one wave per
//                           segment, 64 rows a round: two ballots - "passes" and "continues its predecessor" (the
//                           predecessor by __shfl_up, lane 0 takes the row carried from the round before) - give run
//                           starts and ends by integer bit operations, a segmented wave scan of fixed shape the
//                           sum / min / max of every run. The wave carries the open run from round to round. Run
//                           twice: once to summarise and count, once to write the runs strictly inside the segment.
//   k_episodes_scan_*       the stitch: reduce per 256 summaries / scan the block sums with one workgroup / write
//                           the exclusive fold in front of every segment - trees of fixed shape in LDS, so no
//                           grouping of f64 additions depends on timing.
//   k_episodes_count        1 lane / segment: the attribution rule (episode_attribute) says how many episodes the
//                           segment emits; a scan gives the offsets, one read-back sizes the result.
//   k_episodes_write_ends   1 lane / segment: the episodes of the attribution rule, and the one inside run an interval
//                           segment can have.
// All writes are ordinary vector stores; the only atomics are integer ones (the error word, the passing rows).
#include "mdb_agg_dev.hpp"
#include "mdb_episodes.hpp"
#include "mdb_filter_points.hpp"
#include "mdb_host_side.hpp"
#include "mdb_scan.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace mdb {

constexpr int EPISODE_THREADS = 256;
static_assert(EPISODE_THREADS == FILTER_THREADS, "the waves of a slice are counted as slice_walk counts them");
constexpr int EPISODE_SCAN_ITEMS = 256; // summaries per block of the stitch

struct EpisodeQuery {
    EpisodeRule rule;
    ValueKeys keys;
    int64_t t_lo, t_hi;
    uint32_t n_groups;
};

// Segment i with `rows` rows under the time range, the first of them row `first_row`: per point, or its summary
// and - if its one run lies strictly inside - that run.
struct IntervalClass {
    bool per_point;
    EpisodeSummary summary;
    mdb_episode inner;
};

__device__ __forceinline__ void classify_interval(const DevSegments &s, uint64_t i, const EpisodeQuery &q, uint32_t rows,
                                                  uint64_t first_row, uint32_t group, IntervalClass *out) {
    out->per_point = false;
    out->summary = episode_summary_none();
    out->inner = episode_none();
    if (rows == 0) return;
    const SegInfo info = analyse_segment(s, i);
    const SegDesc &d = info.desc;
    const uint32_t type = d.flags & FLAG_TYPE_MASK;
    if (info.error) return; // (grid_range_plan has reported it)
    uint32_t k_lo = 0, k_hi = 0;
    if (!(d.flags & FLAG_REGULAR) || type == MDB_MACAQUE_V_ID ||
        !regular_index_interval(d.start, d.delta, d.n_total, q.t_lo, q.t_hi, &k_lo, &k_hi)) {
        out->per_point = true;
        return;
    }
    const uint32_t n = k_hi - k_lo + 1;
    // (residual rows in the range; rows the index interval does not explain; steps that do not continue)
    if (k_hi >= d.n_model || n != rows || (n > 1 && (d.delta <= 0 || (uint64_t)d.delta > (uint64_t)q.rule.max_gap))) {
        out->per_point = true;
        return;
    }
    uint32_t ra = k_lo, rb = k_hi;
    const int run_class = model_run(d, type, k_lo, k_hi, q.keys, &ra, &rb);
    if (run_class == RUN_POINTS) {
        out->per_point = true;
        return;
    }
    EpisodeSummary &m = out->summary;
    m.rows = rows;
    m.t_front = d.start + (int64_t)((uint64_t)k_lo * (uint64_t)d.delta);
    m.t_back = d.start + (int64_t)((uint64_t)k_hi * (uint64_t)d.delta);
    m.g_front = m.g_back = group;
    if (run_class != RUN_INTERVAL) return;
    RangeAcc acc;
    model_closed_form(d, type, ra, rb, acc);
    mdb_episode e = episode_none();
    e.first_row = first_row + (ra - k_lo);
    e.count = rb - ra + 1;
    e.t_first = d.start + (int64_t)((uint64_t)ra * (uint64_t)d.delta);
    e.t_last = d.start + (int64_t)((uint64_t)rb * (uint64_t)d.delta);
    e.sum = acc.sum;
    e.min = acc.min;
    e.max = acc.max;
    e.group = group;
    e.first_segment = (uint32_t)i;
    m.passing = e.count;
    if (ra == k_lo) m.head = e;
    if (rb == k_hi) m.tail = e;
    if (ra == k_lo && rb == k_hi) m.whole = 1;
    if (ra != k_lo && rb != k_hi) {
        out->inner = e;
        m.closed = episode_reported(q.rule, e) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(EPISODE_THREADS) void k_episodes_classify(DevSegments s, EpisodeQuery q,
                                                                       const uint32_t *__restrict__ groups,
                                                                       const uint32_t *__restrict__ rows,
                                                                       const unsigned long long *__restrict__ first_row,
                                                                       uint32_t *__restrict__ per_point,
                                                                       EpisodeSummary *__restrict__ summaries,
                                                                       unsigned long long *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * EPISODE_THREADS + threadIdx.x;
    if (i >= s.n) return;
    const uint32_t group = groups ? groups[i] : 0u;
    if (group >= q.n_groups) atomicOr(&words[0], 1ull);
    IntervalClass c;
    classify_interval(s, i, q, rows[i], first_row[i], group, &c);
    per_point[i] = c.per_point ? 1u : 0u;
    summaries[i] = c.summary; // (a per-point segment's is written by k_episodes_points)
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int source) {
    const uint32_t lo = __shfl((uint32_t)v, source, MDB_WAVE);
    const uint32_t hi = __shfl((uint32_t)(v >> 32), source, MDB_WAVE);
    return ((uint64_t)hi << 32) | lo;
}
// Lane `source`'s run in every lane (group and first_segment are the segment's).
__device__ __forceinline__ mdb_episode shfl_episode(const mdb_episode &e, int source) {
    mdb_episode r = e;
    r.first_row = shfl_u64(e.first_row, source);
    r.count = shfl_u64(e.count, source);
    r.t_first = (int64_t)shfl_u64((uint64_t)e.t_first, source);
    r.t_last = (int64_t)shfl_u64((uint64_t)e.t_last, source);
    r.sum = __longlong_as_double((long long)shfl_u64((uint64_t)__double_as_longlong(e.sum), source));
    r.min = __shfl(e.min, source, MDB_WAVE);
    r.max = __shfl(e.max, source, MDB_WAVE);
    return r;
}

// One wave per per-point segment of a slice (rows [first[j], first[j + 1]) of the slice's range grid, gathered
// segment j0 + j, segment `origin` of the batch), 64 rows a round. WRITE false: the segment's summary into
// summaries[origin]. WRITE true: the reported runs strictly inside it - neither its head nor its tail - in order
// from out[offsets[origin] + what the attribution rule puts in front of them] on.
template <bool WRITE>
__global__ __launch_bounds__(EPISODE_THREADS) void k_episodes_points(
    const int64_t *__restrict__ slice_ts, const float *__restrict__ slice_val, const unsigned long long *__restrict__ first,
    uint64_t n_slice, uint64_t j0, Gathered g, EpisodeQuery q, const uint32_t *__restrict__ groups,
    const uint32_t *__restrict__ rows, const unsigned long long *__restrict__ first_row, uint64_t total_rows,
    EpisodeSummary *__restrict__ summaries, const EpisodePrefix *__restrict__ prefixes,
    const unsigned long long *__restrict__ offsets, mdb_episode *__restrict__ out, uint64_t n_out) {
    const int lane = threadIdx.x & (MDB_WAVE - 1);
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long through = below | (1ull << lane);
    const uint64_t waves = (uint64_t)gridDim.x * (EPISODE_THREADS / MDB_WAVE);
    for (uint64_t j = (uint64_t)blockIdx.x * (EPISODE_THREADS / MDB_WAVE) + threadIdx.x / MDB_WAVE; j < n_slice; j += waves) {
        const uint32_t origin = g.origin[j0 + j];
        const uint64_t begin = first[j], end = first[j + 1];
        if (end <= begin) continue; // (never: a per-point segment has rows)
        const uint32_t group = groups ? groups[origin] : 0u;
        const uint64_t segment_row = first_row[origin];
        uint64_t base = 0;
        if (WRITE) {
            const EpisodeSummary own = summaries[origin];
            if (own.closed == 0) continue;
            const bool last = segment_row + rows[origin] == total_rows;
            base = offsets[origin] + episode_attribute(q.rule, prefixes[origin], own, last).before();
        }
        mdb_episode carry = episode_none(), head = episode_none();
        uint64_t closed = 0, passing = 0;
        int64_t t_carried = 0;
        for (uint64_t row0 = begin; row0 < end; row0 += MDB_WAVE) {
            const uint64_t row = row0 + lane;
            const bool valid = row < end;
            const int64_t t = valid ? slice_ts[row] : 0;
            const float v = valid ? slice_val[row] : 0.0f;
            const bool pass = valid && q.keys.pass(v);
            int64_t t_prev = (int64_t)shfl_up_u64((uint64_t)t, 1);
            if (lane == 0) t_prev = t_carried;
            const bool continues = valid && (lane > 0 || row0 > begin) && episode_continues(q.rule, t_prev, group, t, group);
            const unsigned long long passes = __ballot(pass), joins = __ballot(continues);
            const unsigned long long before_passes = (passes << 1) | (carry.count != 0 ? 1ull : 0ull);
            const unsigned long long starts = passes & ~(before_passes & joins);
            // (the carried run ended with the round before if this round's first row does not go on with it)
            if (carry.count != 0 && ((passes & joins) & 1ull) == 0) {
                if (carry.first_row == segment_row) {
                    head = carry;
                } else if (episode_reported(q.rule, carry)) {
                    if (WRITE && lane == 0 && base + closed < n_out) out[base + closed] = carry;
                    closed += 1;
                }
            }
            const unsigned long long extended = (passes & ~starts) >> 1; // lanes whose successor goes on with their run
            const int last_lane = (int)min((uint64_t)(MDB_WAVE - 1), end - 1 - row0);
            const bool stays_open = ((passes >> last_lane) & 1ull) != 0;
            const unsigned long long ends = passes & ~extended & ~(1ull << last_lane);
            // sum / min / max of every run up to its lane: a segmented inclusive scan over the wave (heads: the run
            // starts, and the failing rows, which hold the neutral element)
            const unsigned long long heads = starts | ~passes;
            double sum = pass ? (double)v : 0.0;
            float lowest = pass ? episode_min(FLT_MAX, v) : FLT_MAX, highest = pass ? episode_max(-FLT_MAX, v) : -FLT_MAX;
#pragma unroll
            for (int delta = 1; delta < MDB_WAVE; delta <<= 1) {
                const double sum_up = __longlong_as_double((long long)shfl_up_u64((uint64_t)__double_as_longlong(sum), delta));
                const float lowest_up = __shfl_up(lowest, delta, MDB_WAVE), highest_up = __shfl_up(highest, delta, MDB_WAVE);
                if (lane >= delta && ((heads >> (lane - delta + 1)) & ((1ull << delta) - 1ull)) == 0) {
                    sum = sum_up + sum;
                    lowest = episode_min(lowest_up, lowest);
                    highest = episode_max(highest_up, highest);
                }
            }
            const unsigned long long starts_through = starts & through;
            const bool from_carry = pass && starts_through == 0; // (then every lane up to this one goes on with the carried run)
            const int start_lane = pass && !from_carry ? 63 - __clzll((long long)starts_through) : 0;
            const int64_t t_start = (int64_t)shfl_u64((uint64_t)t, start_lane);
            mdb_episode run = episode_none();
            if (pass) {
                run.first_row = segment_row + (row0 - begin) + (uint64_t)start_lane;
                run.count = (uint64_t)(lane - start_lane + 1);
                run.t_first = t_start;
                run.t_last = t;
                run.sum = sum;
                run.min = lowest;
                run.max = highest;
                if (from_carry) run = episode_join(carry, run);
            }
            run.group = group;
            run.first_segment = origin;
            const bool is_end = ((ends >> lane) & 1ull) != 0;
            const bool is_head = is_end && run.first_row == segment_row;
            const unsigned long long head_ends = __ballot(is_head);
            if (head_ends != 0) head = shfl_episode(run, __ffsll((long long)head_ends) - 1);
            const bool reported = is_end && !is_head && episode_reported(q.rule, run);
            const unsigned long long reports = __ballot(reported);
            if (WRITE && reported) {
                const uint64_t at = base + closed + (uint64_t)__popcll(reports & below);
                if (at < n_out) out[at] = run;
            }
            closed += (uint64_t)__popcll(reports);
            passing += (uint64_t)__popcll(passes);
            const mdb_episode open = shfl_episode(run, last_lane);
            carry = stays_open ? open : episode_none();
            carry.group = group;
            carry.first_segment = origin;
            t_carried = (int64_t)shfl_u64((uint64_t)t, MDB_WAVE - 1);
        }
        if (!WRITE && lane == 0) {
            EpisodeSummary m = episode_summary_none();
            m.rows = end - begin;
            m.t_front = slice_ts[begin];
            m.t_back = slice_ts[end - 1];
            m.g_front = m.g_back = group;
            m.tail = carry;
            m.whole = carry.count != 0 && carry.first_row == segment_row ? 1u : 0u;
            m.head = m.whole ? carry : head;
            m.closed = closed;
            m.passing = passing;
            summaries[origin] = m;
        }
    }
}

// ---- the stitch -------------------------------------------------------------------------------------------------

// Exclusive scan of one summary per thread under the monoid: an up-sweep and a down-sweep over a binary tree in LDS
// (EPISODE_SCAN_ITEMS + 1 entries; the shape depends on nothing but the thread's number). *total: the block's fold.
__device__ __forceinline__ EpisodeSummary block_scan_summaries(EpisodeSummary *lds, const EpisodeRule &rule,
                                                               const EpisodeSummary &mine, EpisodeSummary *total) {
    const uint32_t t = threadIdx.x;
    lds[t] = mine;
    __syncthreads();
    for (uint32_t stride = 1; stride < EPISODE_SCAN_ITEMS; stride <<= 1) {
        const uint32_t at = (t + 1) * 2 * stride - 1;
        if (at < EPISODE_SCAN_ITEMS) lds[at] = episode_combine(rule, lds[at - stride], lds[at]);
        __syncthreads();
    }
    if (t == 0) {
        lds[EPISODE_SCAN_ITEMS] = lds[EPISODE_SCAN_ITEMS - 1];
        lds[EPISODE_SCAN_ITEMS - 1] = episode_summary_none();
    }
    __syncthreads();
    for (uint32_t stride = EPISODE_SCAN_ITEMS / 2; stride >= 1; stride >>= 1) {
        const uint32_t at = (t + 1) * 2 * stride - 1;
        if (at < EPISODE_SCAN_ITEMS) {
            const EpisodeSummary left = lds[at - stride];
            lds[at - stride] = lds[at];                       // the left child: what precedes the node
            lds[at] = episode_combine(rule, lds[at], left);   // the right child: that, then the left child's fold
        }
        __syncthreads();
    }
    const EpisodeSummary result = lds[t];
    *total = lds[EPISODE_SCAN_ITEMS];
    __syncthreads();
    return result;
}

__global__ __launch_bounds__(EPISODE_SCAN_ITEMS) void k_episodes_scan_reduce(const EpisodeSummary *__restrict__ summaries,
                                                                            uint64_t n, EpisodeRule rule,
                                                                            EpisodeSummary *__restrict__ block_sums) {
    __shared__ EpisodeSummary lds[EPISODE_SCAN_ITEMS + 1];
    const uint64_t i = (uint64_t)blockIdx.x * EPISODE_SCAN_ITEMS + threadIdx.x;
    EpisodeSummary total;
    (void)block_scan_summaries(lds, rule, i < n ? summaries[i] : episode_summary_none(), &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// One workgroup: block_sums[b] becomes the fold of the blocks before b. Every thread folds a span of `per`
// consecutive block sums, the spans are scanned as above, then every thread walks its span again.
__global__ __launch_bounds__(EPISODE_SCAN_ITEMS) void k_episodes_scan_block_sums(EpisodeSummary *__restrict__ block_sums,
                                                                                uint64_t n_blocks, EpisodeRule rule) {
    __shared__ EpisodeSummary lds[EPISODE_SCAN_ITEMS + 1];
    const uint64_t per = (n_blocks + EPISODE_SCAN_ITEMS - 1) / EPISODE_SCAN_ITEMS;
    const uint64_t b0 = min((uint64_t)threadIdx.x * per, n_blocks), b1 = min(b0 + per, n_blocks);
    EpisodeSummary span = episode_summary_none();
    for (uint64_t b = b0; b < b1; b++) span = episode_combine(rule, span, block_sums[b]);
    EpisodeSummary total;
    EpisodeSummary running = block_scan_summaries(lds, rule, span, &total);
    for (uint64_t b = b0; b < b1; b++) {
        const EpisodeSummary own = block_sums[b];
        block_sums[b] = running;
        running = episode_combine(rule, running, own);
    }
}

__global__ __launch_bounds__(EPISODE_SCAN_ITEMS) void k_episodes_scan_write(const EpisodeSummary *__restrict__ summaries,
                                                                           uint64_t n, EpisodeRule rule,
                                                                           const EpisodeSummary *__restrict__ block_sums,
                                                                           EpisodePrefix *__restrict__ prefixes) {
    __shared__ EpisodeSummary lds[EPISODE_SCAN_ITEMS + 1];
    const uint64_t i = (uint64_t)blockIdx.x * EPISODE_SCAN_ITEMS + threadIdx.x;
    EpisodeSummary total;
    const EpisodeSummary inside = block_scan_summaries(lds, rule, i < n ? summaries[i] : episode_summary_none(), &total);
    if (i < n) prefixes[i] = episode_prefix_of(episode_combine(rule, block_sums[blockIdx.x], inside));
}

// ---- attribution ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(EPISODE_THREADS) void k_episodes_count(const EpisodeSummary *__restrict__ summaries,
                                                                    const EpisodePrefix *__restrict__ prefixes,
                                                                    const uint32_t *__restrict__ rows,
                                                                    const unsigned long long *__restrict__ first_row,
                                                                    uint64_t n, uint64_t total_rows, EpisodeRule rule,
                                                                    unsigned long long *__restrict__ emitted,
                                                                    unsigned long long *__restrict__ words) {
    __shared__ unsigned long long lds;
    if (threadIdx.x == 0) lds = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * EPISODE_THREADS + threadIdx.x;
    if (i < n) {
        const EpisodeSummary own = summaries[i];
        const bool last = rows[i] != 0 && first_row[i] + rows[i] == total_rows;
        const EpisodeEnds ends = episode_attribute(rule, prefixes[i], own, last);
        emitted[i] = own.rows != 0 ? (unsigned long long)ends.before() + own.closed + ends.emit_open : 0ull;
        if (own.passing) atomicAdd(&lds, (unsigned long long)own.passing);
    }
    __syncthreads();
    if (threadIdx.x == 0 && lds) atomicAdd(&words[1], lds);
}

__global__ __launch_bounds__(EPISODE_THREADS) void k_episodes_write_ends(
    DevSegments s, EpisodeQuery q, const uint32_t *__restrict__ groups, const uint32_t *__restrict__ rows,
    const unsigned long long *__restrict__ first_row, const uint32_t *__restrict__ per_point,
    const EpisodeSummary *__restrict__ summaries, const EpisodePrefix *__restrict__ prefixes,
    const unsigned long long *__restrict__ offsets, uint64_t total_rows, mdb_episode *__restrict__ out, uint64_t n_out) {
    const uint64_t i = (uint64_t)blockIdx.x * EPISODE_THREADS + threadIdx.x;
    if (i >= s.n || rows[i] == 0) return;
    const EpisodeSummary own = summaries[i];
    const bool last = first_row[i] + rows[i] == total_rows;
    const EpisodeEnds ends = episode_attribute(q.rule, prefixes[i], own, last);
    uint64_t at = offsets[i];
    if (ends.emit_incoming) {
        if (at < n_out) out[at] = ends.incoming;
        at++;
    }
    if (ends.emit_first) {
        if (at < n_out) out[at] = ends.first;
        at++;
    }
    if (per_point[i] == 0 && own.closed != 0) { // an interval segment's one run, strictly inside it
        IntervalClass c;
        classify_interval(s, i, q, rows[i], first_row[i], groups ? groups[i] : 0u, &c);
        if (at < n_out) out[at] = c.inner;
    }
    at += own.closed;
    if (ends.emit_open && at < n_out) out[at] = ends.open;
}

namespace {

// The per-segment arrays of one call (SCRATCH_EPISODES_SEGMENTS).
struct EpisodeScratch {
    uint32_t *rows = nullptr;
    unsigned long long *first_row = nullptr; // (n + 1)
    uint32_t *per_point = nullptr;
    EpisodeSummary *summaries = nullptr;
    EpisodePrefix *prefixes = nullptr;
    EpisodeSummary *stitch_sums = nullptr;   // one per block of the stitch
    unsigned long long *emitted = nullptr;
    unsigned long long *offsets = nullptr;   // (n + 1)
    unsigned long long *position = nullptr;  // (n + 1) the gather's scan
    unsigned long long *block_sums = nullptr;
    unsigned long long *words = nullptr;     // [0] a bad group id, [1] the passing rows
};

// What the count leaves for the write.
struct EpisodePass {
    const mdb_segments *in = nullptr;
    const uint32_t *groups = nullptr;
    EpisodeQuery q{};
    EpisodeScratch m;
    FilterPass f;
    uint64_t n_rows = 0, n_passing = 0, n_episodes = 0;
};

uint64_t stitch_blocks(uint64_t n) { return (n + EPISODE_SCAN_ITEMS - 1) / EPISODE_SCAN_ITEMS; }

int episode_scratch(mdb_ctx *ctx, uint64_t n, EpisodeScratch *m) {
    const uint64_t b4 = align_up(n * 4, 256), b8 = align_up((n + 1) * 8, 256);
    const uint64_t summaries = align_up(n * sizeof(EpisodeSummary), 256), prefixes = align_up(n * sizeof(EpisodePrefix), 256);
    const uint64_t stitch = align_up((stitch_blocks(n) + 1) * sizeof(EpisodeSummary), 256);
    const uint64_t sums = align_up(scan_block_sums_bytes(n), 256);
    void *p = nullptr;
    if (scratch_reserve(ctx, SCRATCH_EPISODES_SEGMENTS, 2 * b4 + 4 * b8 + summaries + prefixes + stitch + sums + 512, &p)) return 1;
    Carver scratch(p);
    m->summaries = scratch.take<EpisodeSummary>(n);
    m->prefixes = scratch.take<EpisodePrefix>(n);
    m->stitch_sums = scratch.take<EpisodeSummary>(stitch_blocks(n) + 1);
    m->first_row = scratch.take<unsigned long long>(n + 1);
    m->emitted = scratch.take<unsigned long long>(n + 1);
    m->offsets = scratch.take<unsigned long long>(n + 1);
    m->position = scratch.take<unsigned long long>(n + 1);
    m->block_sums = scratch.take<unsigned long long>(scan_block_sums_bytes(n) / 8);
    m->words = scratch.take<unsigned long long>(4);
    m->rows = scratch.take<uint32_t>(n);
    m->per_point = scratch.take<uint32_t>(n);
    return 0;
}

uint32_t lane_blocks(uint64_t n) { return (uint32_t)((n + EPISODE_THREADS - 1) / EPISODE_THREADS); }

// Pass 1: rows, summaries, the stitch, the emission counts and their offsets. One read-back.
int episodes_count(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *groups, const EpisodeQuery &q, EpisodePass &e) {
    e.in = in;
    e.groups = groups;
    e.q = q;
    const uint64_t n = in->n;
    if (n > 0xffffffffull) return fail("Too many segments for one episodes call.");
    if (episode_scratch(ctx, n, &e.m)) return 1;
    EpisodeScratch &m = e.m;
    if (grid_range_plan(ctx, in, q.t_lo, q.t_hi, &e.n_rows, nullptr, m.rows)) return 1;
    if (n == 0) return 0;
    if (device_exclusive_scan(ctx, ItemsOf<uint32_t>{m.rows}, n, m.first_row, m.block_sums, "k_episodes_scan_rows")) return 1;
    MDB_HIP_CHECK(hipMemsetAsync(m.words, 0, 4 * 8, ctx->stream));
    const DevSegments s = to_dev(in);
    {
        LaunchTimer timer(ctx, "k_episodes_classify");
        hipLaunchKernelGGL(k_episodes_classify, dim3(lane_blocks(n)), dim3(EPISODE_THREADS), 0, ctx->stream, s, q, groups, m.rows,
                           m.first_row, m.per_point, m.summaries, m.words);
    }
    FilterPass &f = e.f;
    f.in = in;
    f.t_lo = q.t_lo;
    f.t_hi = q.t_hi;
    f.keys = q.keys;
    const uint64_t n_rows = e.n_rows;
    if (filter_tested_slices(ctx, f, m.per_point, m.position, m.block_sums, [&](uint64_t j0, uint64_t n_slice) {
            LaunchTimer timer(ctx, "k_episodes_points");
            hipLaunchKernelGGL(k_episodes_points<false>, dim3(slice_walk_blocks(n_slice, 8192)), dim3(EPISODE_THREADS), 0,
                               ctx->stream, f.slice_ts, f.slice_val, f.slice_first, n_slice, j0, f.g, q, groups, m.rows,
                               m.first_row, n_rows, m.summaries, m.prefixes, m.offsets, (mdb_episode *)nullptr, (uint64_t)0);
        }))
        return 1;
    {
        LaunchTimer timer(ctx, "k_episodes_scan");
        const uint64_t n_blocks = stitch_blocks(n);
        hipLaunchKernelGGL(k_episodes_scan_reduce, dim3((uint32_t)n_blocks), dim3(EPISODE_SCAN_ITEMS), 0, ctx->stream, m.summaries,
                           n, q.rule, m.stitch_sums);
        hipLaunchKernelGGL(k_episodes_scan_block_sums, dim3(1), dim3(EPISODE_SCAN_ITEMS), 0, ctx->stream, m.stitch_sums, n_blocks,
                           q.rule);
        hipLaunchKernelGGL(k_episodes_scan_write, dim3((uint32_t)n_blocks), dim3(EPISODE_SCAN_ITEMS), 0, ctx->stream, m.summaries,
                           n, q.rule, m.stitch_sums, m.prefixes);
    }
    {
        LaunchTimer timer(ctx, "k_episodes_count");
        hipLaunchKernelGGL(k_episodes_count, dim3(lane_blocks(n)), dim3(EPISODE_THREADS), 0, ctx->stream, m.summaries, m.prefixes,
                           m.rows, m.first_row, n, n_rows, q.rule, m.emitted, m.words);
    }
    if (device_exclusive_scan(ctx, ItemsOf<unsigned long long>{m.emitted}, n, m.offsets, m.block_sums, "k_episodes_scan_offsets"))
        return 1;
    unsigned long long read_back[3] = {0, 0, 0};
    MDB_HIP_CHECK(hipMemcpyAsync(&read_back[0], m.words, 2 * 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipMemcpyAsync(&read_back[2], m.offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    if (read_back[0] != 0) return fail("A group id is not below n_groups.");
    e.n_passing = read_back[1];
    e.n_episodes = read_back[2];
    return 0;
}

// Pass 2: the e.n_episodes episodes into out (HBM).
int episodes_write(mdb_ctx *ctx, EpisodePass &e, mdb_episode *out) {
    const uint64_t n = e.in->n;
    if (n == 0 || e.n_episodes == 0) return 0;
    EpisodeScratch &m = e.m;
    const EpisodeQuery q = e.q;
    const uint32_t *groups = e.groups;
    const uint64_t n_rows = e.n_rows, n_out = e.n_episodes;
    {
        LaunchTimer timer(ctx, "k_episodes_write_ends");
        hipLaunchKernelGGL(k_episodes_write_ends, dim3(lane_blocks(n)), dim3(EPISODE_THREADS), 0, ctx->stream, to_dev(e.in), q,
                           groups, m.rows, m.first_row, m.per_point, m.summaries, m.prefixes, m.offsets, n_rows, out, n_out);
    }
    FilterPass &f = e.f;
    if (filter_tested_slices(ctx, f, nullptr, m.position, m.block_sums, [&](uint64_t j0, uint64_t n_slice) {
            LaunchTimer timer(ctx, "k_episodes_points_write");
            hipLaunchKernelGGL(k_episodes_points<true>, dim3(slice_walk_blocks(n_slice, 8192)), dim3(EPISODE_THREADS), 0,
                               ctx->stream, f.slice_ts, f.slice_val, f.slice_first, n_slice, j0, f.g, q, groups, m.rows,
                               m.first_row, n_rows, m.summaries, m.prefixes, m.offsets, out, n_out);
        }))
        return 1;
    MDB_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MDB_HIP_CHECK(hipGetLastError());
    return 0;
}

// What can be checked without the device.
int request_check(const mdb_episodes_request *request, EpisodeQuery *q) {
    if (value_keys_fold(&request->filter, &q->keys)) return 1;
    if (request->flags != 0) return fail("flags must be 0 for mdb_episodes*.");
    if (request->max_gap < 0) return fail("max_gap must not be negative.");
    if (request->min_duration < 0) return fail("min_duration must not be negative.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    q->rule = EpisodeRule{request->max_gap, request->min_duration, request->min_count};
    q->t_lo = request->filter.t_lo;
    q->t_hi = request->filter.t_hi;
    q->n_groups = request->n_groups;
    return 0;
}

struct OwnedEpisodes {
    mdb_episodes_result c;
    std::vector<mdb_episode> episodes;
};

} // namespace

} // namespace mdb

using namespace mdb;

extern "C" {

int mdb_episodes_count_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                           const mdb_episodes_request *request, uint64_t *n_episodes, uint64_t *n_rows,
                           uint64_t *n_passing) {
    if (!ctx || !in || !request || !n_episodes || !n_rows || !n_passing)
        return fail("ctx, in, request, n_episodes, n_rows and n_passing must not be NULL.");
    EpisodeQuery q;
    if (request_check(request, &q)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    EpisodePass e;
    if (episodes_count(ctx, in, group_of_segment, q, e)) return 1;
    *n_episodes = e.n_episodes;
    *n_rows = e.n_rows;
    *n_passing = e.n_passing;
    return 0;
}

int mdb_episodes_dev(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment,
                     const mdb_episodes_request *request, mdb_episode *out, uint64_t cap, uint64_t *n_out, uint64_t *n_rows,
                     uint64_t *n_passing) {
    if (!ctx || !in || !request || !n_out || !n_rows || !n_passing)
        return fail("ctx, in, request, n_out, n_rows and n_passing must not be NULL.");
    EpisodeQuery q;
    if (request_check(request, &q)) return 1;
    mdb::CallGuard lock(ctx);
    MDB_HIP_CHECK(hipSetDevice(ctx->device));
    EpisodePass e;
    if (episodes_count(ctx, in, group_of_segment, q, e)) return 1;
    if (e.n_episodes > cap)
        return fail("Output buffer too small: " + std::to_string(e.n_episodes) + " episodes but capacity " +
                    std::to_string(cap) + ".");
    if (e.n_episodes > 0 && !out) return fail("out must not be NULL.");
    if (episodes_write(ctx, e, out)) return 1;
    *n_out = e.n_episodes;
    *n_rows = e.n_rows;
    *n_passing = e.n_passing;
    return 0;
}

int mdb_episodes_list(mdb_ctx *ctx, const mdb_segments *const *inputs, const uint32_t *const *group_of_segment,
                      uint32_t n_inputs, const mdb_episodes_request *request, mdb_episodes_result **out) {
    if (!ctx || !inputs || !request || !out) return fail("ctx, inputs, request and out must not be NULL.");
    EpisodeQuery q;
    if (request_check(request, &q)) return 1;
    std::vector<uint64_t> rows(n_inputs);
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_inputs; k++) {
        if (!inputs[k]) return fail("A batch of the list is NULL.");
        rows[k] = inputs[k]->n;
        n += rows[k];
        if (group_of_segment && group_of_segment[k])
            for (uint64_t i = 0; i < rows[k]; i++)
                if (group_of_segment[k][i] >= q.n_groups) return fail("A group id is not below n_groups.");
    }
    OwnedEpisodes *owned = new OwnedEpisodes();
    owned->c = mdb_episodes_result{nullptr, 0, 0, 0, owned};
    int rc = 0;
    if (n > 0) {
        mdb::CallGuard lock(ctx);
        rc = [&]() -> int {
            MDB_HIP_CHECK(hipSetDevice(ctx->device));
            mdb_segments_owned *dev = nullptr;
            if (upload_segment_list_locked(ctx, inputs, n_inputs, false, &dev)) return 1;
            const uint32_t *groups = nullptr;
            int status = upload_groups(ctx, group_of_segment, rows.data(), n_inputs, n, &groups);
            EpisodePass e;
            if (!status) status = episodes_count(ctx, &dev->seg, groups, q, e);
            if (!status && e.n_episodes > 0) {
                void *p = nullptr;
                status = scratch_reserve(ctx, SCRATCH_EPISODES_OUT, e.n_episodes * sizeof(mdb_episode), &p);
                if (!status) status = episodes_write(ctx, e, static_cast<mdb_episode *>(p));
                if (!status) {
                    owned->episodes.resize(e.n_episodes);
                    hipError_t copied = hipMemcpyAsync(owned->episodes.data(), p, e.n_episodes * sizeof(mdb_episode),
                                                       hipMemcpyDeviceToHost, ctx->stream);
                    if (copied == hipSuccess) copied = hipStreamSynchronize(ctx->stream);
                    if (copied != hipSuccess) status = fail(std::string("Copying the episodes back: ") + hipGetErrorString(copied));
                }
            }
            if (!status) {
                owned->c.episodes = owned->episodes.empty() ? nullptr : owned->episodes.data();
                owned->c.n = e.n_episodes;
                owned->c.n_rows = e.n_rows;
                owned->c.n_passing = e.n_passing;
            }
            mdb_segments_free(dev);
            return status;
        }();
    }
    if (rc) {
        delete owned;
        return 1;
    }
    *out = &owned->c;
    return 0;
}

int mdb_episodes(mdb_ctx *ctx, const mdb_segments *in, const uint32_t *group_of_segment, const mdb_episodes_request *request,
                 mdb_episodes_result **out) {
    if (!in) return fail("in must not be NULL.");
    const uint32_t *const groups[1] = {group_of_segment};
    return mdb_episodes_list(ctx, &in, groups, 1, request, out);
}

void mdb_episodes_result_free(mdb_episodes_result *result) {
    if (result) delete static_cast<OwnedEpisodes *>(result->priv_);
}

} // extern "C"
