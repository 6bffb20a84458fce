// Flat-buffer AdamW: one multi-tensor step over the whole flat fp32 parameter buffer and its
// two moment buffers (torch semantics of torch/optim/adam.py _single_tensor_adam with
// decoupled weight decay, no amsgrad).  As sgd_kernel (optim.hip) it refreshes, in the same
// pass, the shadow copies the MFMA kernels read.
//
// Geometry: that of sgd_kernel - 256 threads, one float4 quad per thread per grid-stride pass,
// grid min(max(ceil(n4 / 256), 1), 2048), the n % 4 tail on the first threads of block 0,
// 16-byte-aligned operands.
//
// Per-step scalars: bias correction needs the step number, and a captured graph replays the
// launch, so nothing that depends on the step travels by value.  coef[k] = {decay, step_size,
// bc2_sqrt, lr} is a device-resident table the host computed in float64 and rounded once
// (ops/adamw.py coef_table); the launch uses entry min(t, n_coef - 1) with t = sched->t
// (types.h SchedState) and advances t itself, by the ticket protocol of the DLR build of
// sgd_kernel: every thread reads t once at entry (an agent-scope load, served by L2) and holds
// it in a register before the block's barrier; thread 0 then takes one relaxed ticket; the
// block that took ticket gridDim.x - 1 knows every block has read t, writes t + 1 and lr_used
// and re-arms the ticket.  The ticket's value is first used after the streaming loop.  A
// shadows-only launch (a.update == 0) is no optimizer step: it reads no table entry and takes
// no ticket.
//
// Element update, all fp32, in this order (w1 = fp32(1 - beta1), b2 = fp32(beta2),
// w2 = fp32(1 - beta2); every line is one rounding unless noted):
//   d   = g                      CLIP: d = g * gscale[0]; maximize: d = -d (exact)
//   p1  = p * decay
//   m'  = fma(w1, d - m, m)                        (d - m rounded, then one fma)
//   v'  = fma(w2 * d, d, b2 * v)                   (w2 * d and b2 * v rounded, then one fma)
//   den = sqrt(v') / bc2_sqrt + eps                (IEEE sqrt, IEEE divide, add)
//   p'  = fma(-step_size, m' / den, p1)            (IEEE divide, then one fma)
// Every multiply-add pair is an explicit fmaf, so the compiler's contraction has nothing left
// to choose; the TU is built without fast-math, so sqrtf and / are the correctly rounded
// expansions (v_sqrt_f32 / v_rcp_f32 seeds with the fma fix-up and v_div_fixup_f32).
#include "kernels/common.h"
#include "kernels/launchers.h"
#include "kernels/shadow.h"

namespace ddp_amd {

// c = {decay, step_size, bc2_sqrt, lr}
__device__ __forceinline__ float adamw_one(float p, float d, float* m, float* v, const AdamArgs& a,
                                           const float4& c) {
  if (a.maximize) d = -d;
  const float p1 = p * c.x;
  const float m1 = fmaf(a.w1, d - *m, *m);
  const float v1 = fmaf(a.w2 * d, d, a.b2 * (*v));
  const float den = sqrtf(v1) / c.z + a.eps;
  *m = m1;
  *v = v1;
  return fmaf(-c.y, m1 / den, p1);
}

template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ mbuf, float* __restrict__ vbuf,
                                                    long n, AdamArgs a, ShadowSet sh,
                                                    const float* __restrict__ gscale,
                                                    const float4* __restrict__ coef, int n_coef,
                                                    SchedState* __restrict__ sched) {
  float gs = 1.f;
  if constexpr (CLIP) gs = gscale[0];
  int t = 0, ticket = -1;
  float4 c = {1.f, 0.f, 1.f, 0.f};
  if (a.update) {
    t = __hip_atomic_load(&sched->t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(t) : : "memory");  // t is in a register from here on
    t = __builtin_amdgcn_readfirstlane(t);
    c = coef[t < 0 ? 0 : (t < n_coef ? t : n_coef - 1)];
    __syncthreads();  // every wave of the block has read t
    if (threadIdx.x == 0)
      ticket = __hip_atomic_fetch_add(&sched->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += stride) {
    const long i = q << 2;
    float4 w = reinterpret_cast<const float4*>(p)[q];
    if (a.update) {
      float4 d = reinterpret_cast<const float4*>(g)[q];
      float4 m = reinterpret_cast<const float4*>(mbuf)[q];
      float4 v = reinterpret_cast<const float4*>(vbuf)[q];
      if constexpr (CLIP) { d.x *= gs; d.y *= gs; d.z *= gs; d.w *= gs; }
      w.x = adamw_one(w.x, d.x, &m.x, &v.x, a, c);
      w.y = adamw_one(w.y, d.y, &m.y, &v.y, a, c);
      w.z = adamw_one(w.z, d.z, &m.z, &v.z, a, c);
      w.w = adamw_one(w.w, d.w, &m.w, &v.w, a, c);
      reinterpret_cast<float4*>(p)[q] = w;
      reinterpret_cast<float4*>(mbuf)[q] = m;
      reinterpret_cast<float4*>(vbuf)[q] = v;
    }
    shadow_quad(sh, i, w);
  }
  // scalar tail
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    float w = p[i];
    if (a.update) {
      float d = g[i], m = mbuf[i], v = vbuf[i];
      if constexpr (CLIP) d *= gs;
      w = adamw_one(w, d, &m, &v, a, c);
      p[i] = w;
      mbuf[i] = m;
      vbuf[i] = v;
    }
    shadow_one(sh, i, w);
  }
  if (threadIdx.x == 0 && ticket == (int)gridDim.x - 1) {  // the last arrival: every block has read t
    __hip_atomic_store(&sched->t, t < 0x7fffffff ? t + 1 : t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&sched->lr_used, c.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&sched->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool CLIP>
static void adamw_launch(unsigned grid, hipStream_t s, float* p, const float* g, float* mbuf, float* vbuf,
                         long n, const AdamArgs& a, const ShadowSet& sh, const float* gscale,
                         const float* coef, int n_coef, SchedState* sched) {
  hipLaunchKernelGGL((adamw_kernel<CLIP>), dim3(grid), dim3(256), 0, s, p, g, mbuf, vbuf, n, a, sh, gscale,
                     reinterpret_cast<const float4*>(coef), n_coef, sched);
}

void adamw_step(float* p, const float* g, float* mbuf, float* vbuf, long n, const AdamArgs& a,
                const ShadowSet& sh, hipStream_t s, const float* gscale, const float* coef, int n_coef,
                SchedState* sched) {
  // 16-byte accesses need 16-byte-aligned buffers (torch allocations and flat views are)
  const long blocks = ((n >> 2) + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 2048 ? (blocks > 0 ? blocks : 1) : 2048);
  auto launch = gscale ? adamw_launch<true> : adamw_launch<false>;
  launch(grid, s, p, g, mbuf, vbuf, n, a, sh, gscale, coef, n_coef, sched);
}

}  // namespace ddp_amd
