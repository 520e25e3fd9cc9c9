// components.hpp -- connected components by min-hooking with shortcutting (the shape of FastSV), the part that does not depend on
// the graph.  Per round gf = f[f], then for every edge (u, v) f[f[u]] <- min(., gf[v]), f[u] <- min(., gf[v]), and
// f[u] <- min(., gf[u]).  f only ever decreases, f[u] <= u names a node of u's component throughout, and the only fixed point is
// f[u] = the lowest index of u's component: the int32 atomicMin / atomicAdd here change the road, never the result.  A label of -1
// marks a node outside the graph (a grid point outside the solid); it is never hooked in and never counted.
//
// A user brings its init kernel (f[u] = u or -1) and its hook kernel (its neighbourhood, cc_lower for every edge); the host loop is
// cc_run in dsdf_api.hip.  Users: meshtopo.hpp (faces under the mate relation), tetmesh.hpp (grid points over the Kuhn edges).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blockops.hpp"

namespace dsdf {

constexpr int CC_BLOCK = 256;            // lanes per workgroup of the kernels of this file
constexpr int MT_CC_GROUP = 4;           // rounds enqueued between two reads of the change flags on the host (both users)

__global__ __launch_bounds__(CC_BLOCK) void cc_flags_kernel(int32_t* __restrict__ flags) {
  if (threadIdx.x < MT_CC_GROUP) flags[threadIdx.x] = 0;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_grand_kernel(const int32_t* __restrict__ f, int64_t n, int32_t* __restrict__ gf) {
  const int64_t u = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
  if (u >= n) return;
  const int fu = f[u];
  gf[u] = fu < 0 ? -1 : f[clamp_index(fu, n)];
}

// f[at] <- min(f[at], g); true if that lowered it.  f is read plainly while other lanes lower it: a stale value is a larger one,
// still a node of the same component, and costs at most an atomic that changes nothing.  g comes from gf, constant during the
// launch, and is >= 0, so a label never becomes negative.
__device__ __forceinline__ bool cc_lower(int32_t* f, int64_t at, int g) { return g < f[at] && atomicMin(&f[at], g) > g; }

__global__ __launch_bounds__(CC_BLOCK) void cc_zero_kernel(int32_t* __restrict__ size, int64_t n) {
  const int64_t u = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
  if (u < n) size[u] = 0;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_size_kernel(const int32_t* __restrict__ label, int64_t n, int32_t* __restrict__ size) {
  const int64_t u = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
  if (u < n && label[u] >= 0) atomicAdd(&size[clamp_index(label[u], n)], 1);
}

}  // namespace dsdf
