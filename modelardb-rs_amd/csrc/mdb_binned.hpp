// mdb_binned.hpp - the moments of one field per value cell of another (mdb_binned_buckets*): per date_bin bucket,
// group and cell of x the count, the mean and m2 of the y values of the pairs whose x value falls in the cell.
//
// Plain C++ (no HIP type): the checks every form makes before it touches the device, shared by mdb_binned.hip, by the
// host entry points (mdb_binned_host.cpp) and by the check program tests/binned_host, which runs them under the CPU
// sanitizers. The arithmetic is that of mdb_moments.hpp, unchanged: a run - a maximal stretch of consecutive pairs of
// one x segment inside one bucket and one cell of x - is summed around its first y value (moments_point,
// moments_finish), and runs meet only in moments_merge.
#pragma once

#include "mdb_hist.hpp"
#include "mdb_moments.hpp"

namespace mdb {

// The edges' keys (those of mdb_hist_buckets*) and the request; *n_cells = n_groups * n_buckets * (n_edges + 1).
inline int binned_arguments_check(const mdb_bucket_request *request, const float *edges, uint32_t n_edges,
                                  std::vector<int32_t> *edge_keys, uint64_t *n_cells) {
    if (hist_edge_keys(edges, n_edges, edge_keys)) return 1;
    if (request->which_mask != 0) return fail("which_mask must be 0 for mdb_binned_buckets*.");
    if (request->width <= 0) return fail("The bucket width must be positive.");
    if (request->n_groups == 0) return fail("n_groups must be at least 1.");
    const unsigned __int128 rows = (unsigned __int128)request->n_groups * request->n_buckets;
    if (rows * ((uint64_t)n_edges + 1) > (unsigned __int128)(UINT64_MAX / 32))
        return fail("n_groups * n_buckets * n_cells overflows.");
    *n_cells = (uint64_t)rows * ((uint64_t)n_edges + 1);
    return 0;
}

// mdb_binned.hip: the host batches of the two lists uploaded (a batch that is in both lists once) and folded into the
// caller's cells (the arguments checked, xs not empty). The only step of the host forms that needs the device.
int binned_list_run(mdb_ctx *ctx, const mdb_segments *const *xs, uint32_t n_x, const mdb_segments *const *ys, uint32_t n_y,
                    const uint32_t *const *group_of_segment_x, const mdb_bucket_request *request,
                    const std::vector<int32_t> &edge_keys, uint64_t n_cells, mdb_moments_cell *inout);

} // namespace mdb
