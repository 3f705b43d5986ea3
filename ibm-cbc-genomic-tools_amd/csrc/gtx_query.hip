// Kernel of the per-query hits (see gtx_query.h).
#include <algorithm>
#include "gtx_query.h"

namespace gtx {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

__global__ __launch_bounds__(kThreads) void query_narrow_kernel(const long long *__restrict__ cnt, long long n, unsigned *__restrict__ hits)
{
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < n; t += (long long)gridDim.x * kThreads) hits[t] = (unsigned)cnt[t];
}

}  // namespace

hipError_t launch_query_narrow(const long long *cnt, long long n, unsigned *hits, hipStream_t st)
{
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<long long>((n + kThreads - 1) / kThreads, kMaxBlocks);
  hipLaunchKernelGGL(query_narrow_kernel, dim3(grid), dim3(kThreads), 0, st, cnt, n, hits);
  return hipGetLastError();
}

}  // namespace gtx
