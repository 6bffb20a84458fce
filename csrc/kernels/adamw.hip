// Flat-buffer AdamW: one multi-tensor step over the whole flat fp32 parameter buffer and its
// two moment buffers (torch semantics of torch/optim/adam.py _single_tensor_adam with
// decoupled weight decay, no amsgrad).  As sgd_kernel (optim.hip) it refreshes, in the same
// pass, the shadow copies the MFMA kernels read.  Geometry, the streaming pass and the CLIP
// multiply are flat_step.h's (flat_stream), shared with sgd_kernel and lars_kernel.
//
// Per-step scalars: bias correction needs the step number, and a captured graph replays the
// launch, so nothing that depends on the step travels by value.  coef[k] = {decay, step_size,
// bc2_sqrt, lr} is a device-resident table the host computed in float64 and rounded once
// (ops/adamw.py coef_table); the launch uses entry min(t, n_coef - 1) with t = sched->t
// (types.h SchedState) and advances t itself, by the schedule protocol of flat_step.h.
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
#include "kernels/flat_step.h"
#include "kernels/launchers.h"

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

// adamw_kernel's rule for flat_stream: adamw_one, both moment buffers read and written
struct AdamwRule {
  float* mbuf;
  float* vbuf;
  AdamArgs a;
  float4 c;
  __device__ __forceinline__ float4 quad(long q, float4 w, float4 d) const {
    float4 m = reinterpret_cast<const float4*>(mbuf)[q];
    float4 v = reinterpret_cast<const float4*>(vbuf)[q];
    w.x = adamw_one(w.x, d.x, &m.x, &v.x, a, c);
    w.y = adamw_one(w.y, d.y, &m.y, &v.y, a, c);
    w.z = adamw_one(w.z, d.z, &m.z, &v.z, a, c);
    w.w = adamw_one(w.w, d.w, &m.w, &v.w, a, c);
    reinterpret_cast<float4*>(mbuf)[q] = m;
    reinterpret_cast<float4*>(vbuf)[q] = v;
    return w;
  }
  __device__ __forceinline__ float one(long i, float w, float d) const {
    float m = mbuf[i], v = vbuf[i];
    w = adamw_one(w, d, &m, &v, a, c);
    mbuf[i] = m;
    vbuf[i] = v;
    return w;
  }
};

// There is no DLR parameter: with a.update the kernel always reads the table, and lr_used is
// the entry's c.w.  A shadows-only launch (a.update == 0) is no optimizer step: it reads no
// table entry and takes no ticket, so t does not advance (sgd_kernel<.., true> differs).
template <bool CLIP>
__global__ __launch_bounds__(FLAT_THREADS) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ mbuf, float* __restrict__ vbuf, long n, AdamArgs a, ShadowSet sh,
    const float* __restrict__ gscale, const float4* __restrict__ coef, int n_coef, SchedState* __restrict__ sched) {
  float gs = 1.f;
  if constexpr (CLIP) gs = gscale[0];
  int t = 0, ticket = -1;
  float4 c = {1.f, 0.f, 1.f, 0.f};
  if (a.update) {
    t = sched_read_t(sched);
    c = coef[sched_index(t, n_coef)];
    __syncthreads();  // every wave of the block has read t
    ticket = sched_ticket(sched);
  }
  flat_stream<CLIP>(p, g, n, a.update, gs, sh, AdamwRule{mbuf, vbuf, a, c});
  sched_finish(sched, t, ticket, c.w);
}

void adamw_step(float* p, const float* g, float* mbuf, float* vbuf, long n, const AdamArgs& a,
                const ShadowSet& sh, hipStream_t s, const float* gscale, const float* coef, int n_coef,
                SchedState* sched) {
  hipLaunchKernelGGL(gscale ? adamw_kernel<true> : adamw_kernel<false>, dim3(flat_grid(n)), dim3(FLAT_THREADS), 0, s, p, g,
                     mbuf, vbuf, n, a, sh, gscale, reinterpret_cast<const float4*>(coef), n_coef, sched);
}

}  // namespace ddp_amd
