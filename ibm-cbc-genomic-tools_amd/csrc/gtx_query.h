// Per-query hits (gtx_query_hits / gtx_query_hits_device, include/gtx.h): for every query of a batch in HBM the number of
// reference regions it overlaps -- the length of its segment in the overlap join (gtx_join.h).  The counts are the join's own:
// launch_join_count leaves them in 64 bits on its way to the offsets, and a query has at most n_refs < 2^31 pairs.
#pragma once
#include <hip/hip_runtime.h>

namespace gtx {

// hits[i] = (unsigned)cnt[i]: the counts launch_join_count leaves
hipError_t launch_query_narrow(const long long *cnt, long long n, unsigned *hits, hipStream_t st);

}  // namespace gtx
