// mdb_roll_host.cpp - the entry points of the rolling windows that need no device: mdb_roll_windows and mdb_roll_cells
// (host arithmetic, no context, no GPU), and mdb_roll_cells_dev up to the point where the device is needed
// (roll_dev_run: mdb_roll.hip). Plain C++, no HIP type: the check program tests/roll_host builds this file with g++
// under the CPU sanitizers against a stand-in for the device step.
#include "mdb_roll.hpp"

using namespace mdb;

extern "C" {

int mdb_roll_windows(const mdb_roll_request *request, uint64_t *n_windows) {
    if (!request || !n_windows) return fail("request and n_windows must not be NULL.");
    RollPlan plan;
    if (roll_plan(request, &plan)) return 1;
    *n_windows = plan.n_windows;
    return 0;
}

int mdb_roll_cells(const mdb_roll_request *request, const void *cells, void *out, uint64_t capacity_cells) {
    RollPlan plan;
    if (roll_check(request, cells, out, capacity_cells, &plan)) return 1;
    if (plan.nothing) return 0;
    const mdb_roll_request q = *request;
    return roll_dispatch(q.kind, [&](auto ops) {
        using Ops = decltype(ops);
        using Cell = typename Ops::Cell;
        return roll_host<Ops>(q, plan, static_cast<const Cell *>(cells), static_cast<Cell *>(out));
    });
}

int mdb_roll_cells_dev(mdb_ctx *ctx, const mdb_roll_request *request, const void *cells, void *out,
                       uint64_t capacity_cells) {
    if (!ctx) return fail("ctx must not be NULL.");
    RollPlan plan;
    if (roll_check(request, cells, out, capacity_cells, &plan)) return 1;
    if (plan.nothing) return 0;
    return roll_dev_run(ctx, request, &plan, cells, out);
}

} // extern "C"
