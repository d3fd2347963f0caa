// mdb_agg_merge.hpp - the merge rule of mdb_agg_state, for host and device: what mdb_agg_merge_n, mdb_agg_all_reduce
// (mdb_comm.hip) and the rolling windows (mdb_roll.hpp) apply. Plain C++ (no HIP type).
#pragma once

#include "../../include/mdb_format.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MDB_AGG_MERGE_FN __host__ __device__ __forceinline__
#else
#define MDB_AGG_MERGE_FN inline
#endif

namespace mdb {

// Fold `from` into `into` exactly as the accumulators fold a batch into their state
// (model_simple_aggregates.rs:355 count, :398-401 min, :441-444 max, :501-510 sum): NaN partial
// extrema are skipped the way f32::min / f32::max skip them.
MDB_AGG_MERGE_FN void agg_state_merge(mdb_agg_state &into, const mdb_agg_state &from) {
    into.sum += from.sum;
    into.count += from.count;
    if (!(from.min != from.min) && (into.min != into.min || from.min < into.min)) into.min = from.min;
    if (!(from.max != from.max) && (into.max != into.max || from.max > into.max)) into.max = from.max;
}

} // namespace mdb
