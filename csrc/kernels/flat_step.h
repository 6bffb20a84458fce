// What sgd_kernel (optim.hip), adamw_kernel (adamw.hip) and lars_kernel (lars.hip) share.  Each is
// a rule (below) plus a short body: gscale, schedule entry, flat_stream, schedule finish.
// Geometry: 256 threads, one 16-byte quad per thread per grid-stride pass, grid
// min(max(ceil(n4 / 256), 1), 2048) with n4 = n / 4 quads; the n % 4 tail runs on the first
// threads of block 0.  Operands are 16-byte aligned (torch allocations and flat views are).
#pragma once

#include "kernels/common.h"
#include "kernels/shadow.h"

namespace ddp_amd {

constexpr int FLAT_THREADS = 256;  // (not blockDim.x: the three launchers are the kernels' only callers)

inline unsigned flat_grid(long n) {
  const long blocks = ((n >> 2) + FLAT_THREADS - 1) / FLAT_THREADS;
  return (unsigned)(blocks < 2048 ? (blocks > 0 ? blocks : 1) : 2048);
}

// ---- the schedule protocol -------------------------------------------------------------------
// The per-step scalars (the learning rate; AdamW's coefficient entry) are table[min(t, n - 1)]
// with t = sched->t read from device memory at run time (types.h SchedState), and the launch
// itself advances t, so eager steps and replays of a captured graph share one counter.
//   1. sched_read_t: every thread reads t once at entry - an agent-scope load: served by L2,
//      never by an L1 line of an earlier launch - and holds it in a register (the wait consumes
//      it) before
//   2. the block's barrier, a __syncthreads() in the kernel itself (lars_kernel shares it with
//      its LDS table fill): every wave of the block has read t.
//   3. sched_ticket: only then does thread 0 take a ticket, one relaxed agent-scope add per
//      block (the pattern of bn_tail.h last_arrival).  The ticket publishes nothing but "this
//      block has read t", so it needs no fence.
//   4. sched_finish, after the streaming pass: the block that took ticket gridDim.x - 1 knows
//      every block has read t; it writes t + 1 (saturating) and lr_used and re-arms the ticket.
//      The next launch sees t through the launch boundary.
// The ticket's value is first used in step 4, after the streaming loop, so thread 0's wave
// issues its loads behind the atomic instead of waiting for it.
__device__ __forceinline__ int sched_read_t(const SchedState* sched) {
  int t = __hip_atomic_load(&sched->t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(t) : : "memory");  // t is in a register from here on
  return __builtin_amdgcn_readfirstlane(t);
}

__device__ __forceinline__ int sched_index(int t, int n) { return t < 0 ? 0 : (t < n ? t : n - 1); }

// after the block's barrier; -1 on every thread but thread 0, and on all without a ticket taken
__device__ __forceinline__ int sched_ticket(SchedState* sched) {
  int ticket = -1;
  if (threadIdx.x == 0)
    ticket = __hip_atomic_fetch_add(&sched->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return ticket;
}

__device__ __forceinline__ void sched_finish(SchedState* sched, int t, int ticket, float lr_used) {
  if (threadIdx.x == 0 && ticket == (int)gridDim.x - 1) {  // the last arrival: every block has read t
    __hip_atomic_store(&sched->t, t < 0x7fffffff ? t + 1 : t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&sched->lr_used, lr_used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&sched->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- the streaming pass ----------------------------------------------------------------------
// Every quad of p, then the tail: with `update` the new parameters are rule(parameters, gradient)
// and are stored; with or without, the shadows of the (new) parameters are refreshed.
// CLIP: the gradient is g[i] * gs (one fp32 multiply - the rounding of scaling the gradient
// buffer in place, which is not rewritten); gs is the clip coefficient that grad_sqnorm_kernel
// left in device memory, read once per thread by the kernel, so a captured graph replays with
// each step's own coefficient.
// Rule: a small by-value struct with
//   float4 quad(long q, float4 v, float4 d)   quad q = flat elements [4 q, 4 q + 4)
//   float  one(long i, float v, float d)      flat element i (the tail)
// Each loads its own state (every load before the first dependent use), applies the element
// function, stores its state and returns the new parameters.
template <bool CLIP, class Rule>
__device__ __forceinline__ void flat_stream(float* __restrict__ p, const float* __restrict__ g, long n,
                                            int update, float gs, const ShadowSet& sh, Rule rule) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * FLAT_THREADS;
  for (long q = (long)blockIdx.x * FLAT_THREADS + threadIdx.x; q < n4; q += stride) {
    float4 v = reinterpret_cast<const float4*>(p)[q];
    if (update) {
      float4 d = reinterpret_cast<const float4*>(g)[q];
      if constexpr (CLIP) { d.x *= gs; d.y *= gs; d.z *= gs; d.w *= gs; }
      v = rule.quad(q, v, d);
      reinterpret_cast<float4*>(p)[q] = v;
    }
    shadow_quad(sh, q << 2, v);
  }
  // scalar tail
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    float v = p[i];
    if (update) {
      float d = g[i];
      if constexpr (CLIP) d *= gs;
      v = rule.one(i, v, d);
      p[i] = v;
    }
    shadow_one(sh, i, v);
  }
}

}  // namespace ddp_amd
