// The plane stage of the reduction tree of planes.h -- the one kernel that adds the fp64 partials of a plane in chunk order --
// and the host side of a launch by row chunks: its plan, the checks every such entry makes, and the second launch.
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;

// partial[(plane * n_chunks + chunk) * n_out + j] -> sums[plane * n_out + j]; one lane per (plane, j).
__global__ __launch_bounds__(kThreads) void finish_partials_kernel(const double* __restrict__ partial, int n_planes,
                                                                   int n_chunks, int n_out, double* __restrict__ sums) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)n_planes * n_out) return;
  const int64_t plane = i / n_out;
  const int j = (int)(i % n_out);
  const double* p = partial + plane * n_chunks * n_out + j;
  double v = p[0];
  for (int k = 1; k < n_chunks; ++k) v += p[(int64_t)k * n_out];
  sums[i] = v;
}

}  // namespace

int plan_chunks(const char* name, int n_planes, int n_lat, int n_lon, int chunk_elems, int waves, ChunkPlan* plan) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1 && n_lon >= 1, "%s: bad sizes (planes %d, grid %d x %d)", name, n_planes, n_lat,
                   n_lon);
  *plan = chunk_plan(n_planes, n_lat, n_lon, chunk_elems, waves);
  AURORA_CHECK_ARG(plan->groups <= 0x7fffffff, "%s: too many planes for one launch (%d planes x %lld row chunks)", name,
                   n_planes, (long long)plan->n_chunks);
  return AURORA_OK;
}

int finish_partials(const char* name, const double* partial, int n_planes, int n_chunks, int n_out, double* sums,
                    hipStream_t stream) {
  const unsigned grid = (unsigned)(((int64_t)n_planes * n_out + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(finish_partials_kernel, dim3(grid), dim3(kThreads), 0, stream, partial, n_planes, n_chunks, n_out, sums);
  char what[64];
  snprintf(what, sizeof(what), "%s (finish)", name);
  return check_launch(what);
}

}  // namespace aurora
