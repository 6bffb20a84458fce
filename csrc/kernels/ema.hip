// Exponential moving average of the flat fp32 parameters, and the exchange that puts the
// averaged weights in the model's place for evaluation.
//
// ema_kernel: a rule on flat_stream (flat_step.h) with the flat EMA buffer e in the place of
// the parameters and the live flat parameters p in the place of the (const) gradient.  Element
// update, fp32:
//   e' = fma(om, p - e, e)                            (p - e rounded, then one fma)
// with om = fp32(1 - decay_k).  Written with fmaf, so the rounding does not depend on contraction
// flags.  The EMA has no shadow copies of its own (an empty ShadowSet) and no CLIP build.
//   WARM = false: a constant decay; om travels by value and block 0's thread 0 counts the launch
//     in num_updates[0], the way sgd_kernel bumps step_ctr.  Nothing in the launch reads that word.
//   WARM = true:  decay_k = min(decay, (1 + k) / (10 + k)) for update k = 0, 1, ...: om is
//     table[min(t, n_table - 1)] with t = sched->t, a SchedState of the EMA's own (with gradient
//     accumulation or AdamW the optimizer's counter means something else), read and advanced by
//     the schedule protocol of flat_step.h - a captured step graph replays every update with its
//     own decay.  sched->t is the number of updates.
//
// ema_swap_kernel: exchanges p and e quad by quad (tail included) and refreshes the shadows of
// the new p in the same pass, with the writers the optimizers use (shadow.h).  A pure exchange:
// two launches restore both buffers and every shadow bit for bit.  flat_stream takes its second
// operand as const __restrict__, so this is a short loop of its own over the same geometry.
#include "kernels/common.h"
#include "kernels/flat_step.h"
#include "kernels/launchers.h"
#include "kernels/shadow.h"

namespace ddp_amd {

__device__ __forceinline__ float ema_one(float e, float p, float om) { return fmaf(om, p - e, e); }

// ema_kernel's rule for flat_stream: v is the EMA, d the live parameters; no state of its own
struct EmaRule {
  float om;
  __device__ __forceinline__ float4 quad(long, float4 v, float4 d) const {
    v.x = ema_one(v.x, d.x, om);
    v.y = ema_one(v.y, d.y, om);
    v.z = ema_one(v.z, d.z, om);
    v.w = ema_one(v.w, d.w, om);
    return v;
  }
  __device__ __forceinline__ float one(long, float v, float d) const { return ema_one(v, d, om); }
};

// The WARM = false build carries the three schedule arguments unused, the WARM = true build
// num_updates (its counter is sched->t).
template <bool WARM>
__global__ __launch_bounds__(FLAT_THREADS) void ema_kernel(float* __restrict__ e, const float* __restrict__ p, long n,
    float om, int* __restrict__ num_updates, const float* __restrict__ table, int n_table,
    SchedState* __restrict__ sched) {
  int t = 0, ticket = -1;
  if constexpr (WARM) {
    t = sched_read_t(sched);
    om = table[sched_index(t, n_table)];
    __syncthreads();  // every wave of the block has read t
    ticket = sched_ticket(sched);
  }
  ShadowSet none;
  none.count = 0;
  flat_stream<false>(e, p, n, 1, 1.f, none, EmaRule{om});
  if constexpr (WARM) {
    sched_finish(sched, t, ticket, om);
  } else {
    if (blockIdx.x == 0 && threadIdx.x == 0) num_updates[0] += 1;
  }
}

__global__ __launch_bounds__(FLAT_THREADS) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ e, long n,
                                                                ShadowSet sh) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * FLAT_THREADS;
  for (long q = (long)blockIdx.x * FLAT_THREADS + threadIdx.x; q < n4; q += stride) {
    const float4 vp = reinterpret_cast<const float4*>(p)[q];
    const float4 ve = reinterpret_cast<const float4*>(e)[q];
    reinterpret_cast<float4*>(p)[q] = ve;
    reinterpret_cast<float4*>(e)[q] = vp;
    shadow_quad(sh, q << 2, ve);
  }
  // scalar tail
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    const float vp = p[i], ve = e[i];
    p[i] = ve;
    e[i] = vp;
    shadow_one(sh, i, ve);
  }
}

void ema_step(float* e, const float* p, long n, float om, int* num_updates, hipStream_t s, const float* table,
              int n_table, SchedState* sched) {
  const bool warm = sched != nullptr && table != nullptr && n_table > 0;
  hipLaunchKernelGGL(warm ? ema_kernel<true> : ema_kernel<false>, dim3(flat_grid(n)), dim3(FLAT_THREADS), 0, s, e, p,
                     n, om, num_updates, table, n_table, sched);
}

void ema_swap(float* p, float* e, long n, const ShadowSet& sh, hipStream_t s) {
  hipLaunchKernelGGL(ema_swap_kernel, dim3(flat_grid(n)), dim3(FLAT_THREADS), 0, s, p, e, n, sh);
}

}  // namespace ddp_amd
