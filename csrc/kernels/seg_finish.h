// What seg_sqnorm_kernel (lars.hip) and lamb_moments_kernel (lamb.hip) share after their item
// loops: step 5 of the summation order in lars.hip's header.  The block that arrived last calls
// seg_finish: wave v takes tensors v, v + 4, ...; lane j sums the tensor's item partials j, j + 64,
// ... sequentially from +0.0f (agent-scope loads, no fence), then wave_sum gives both sums ->
// sums[s]; lane 0 hands them to `entry`, which returns the tensor's trust[s].  One body, so the
// first sum of either kernel is the other's bit for bit.
#pragma once

#include "kernels/common.h"
#include "kernels/launchers.h"

namespace ddp_amd {

__device__ __forceinline__ float2 ld_agent2(const float2* p) {
  const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_float2(__uint_as_float((unsigned)v), __uint_as_float((unsigned)(v >> 32)));
}

// entry(seg, S_a, S_b) -> float4, called by lane 0 only
template <class Entry>
__device__ __forceinline__ void seg_finish(const LarsSeg* __restrict__ segs, int n_seg, int n_items,
                                           const float2* __restrict__ partials, float2* __restrict__ sums,
                                           float4* __restrict__ trust, Entry entry) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int s = wave; s < n_seg; s += 4) {
    const LarsSeg sg = segs[s];
    int ni = sg.n_items;
    if (sg.item0 < 0 || ni < 0 || (long)sg.item0 + ni > n_items) ni = 0;
    float a = 0.f, b = 0.f;
    for (int k = lane; k < ni; k += 64) {
      const float2 p = ld_agent2(partials + sg.item0 + k);
      a += p.x;
      b += p.y;
    }
    const float Sa = wave_sum(a), Sb = wave_sum(b);
    if (lane == 0) {
      sums[s] = make_float2(Sa, Sb);
      trust[s] = entry(sg, Sa, Sb);
    }
  }
}

}  // namespace ddp_amd
