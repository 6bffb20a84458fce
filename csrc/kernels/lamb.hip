// Flat-buffer LAMB (layer-wise adaptive moments): Adam's update direction, scaled per tensor by
// the trust ratio |w| / |u| of the weights and of the UPDATE u - not of the gradient, so the
// ratio cannot come from seg_sqnorm_kernel (lars.hip): the new moments must exist before the
// norm does.  Two launches per step, both replayable by a captured graph:
//   lamb_moments_kernel<CLIP>  new moments stored, per-tensor S_w = sum w^2 and S_u = sum u^2,
//                              trust[s] = {phi, wd, |w|, |u|} left in device memory;
//   lamb_apply_kernel          a rule on flat_stream (flat_step.h): w' from w, m', v' and the
//                              table, shadow refresh included; advances the step counter.
//
// Definition.  For tensor i with flat elements w, g, m, v at step k = t + 1, all fp32, every
// line one rounding unless noted (w1 = fp32(1 - beta1), b2 = fp32(beta2), w2 = fp32(1 - beta2)):
//   d   = g                       CLIP: d = g * gscale[0]; maximize: d = -d (exact)
//   m'  = fma(w1, d - m, m)       (d - m rounded, then one fma)              adamw_one's lines
//   v'  = fma(w2 * d, d, b2 * v)  (w2 * d and b2 * v rounded, then one fma)
//   den = sqrt(v') / bc2_sqrt + eps          (IEEE sqrt, IEEE divide, add)
//   r   = (m' / den) * ibc1                  (IEEE divide, multiply)  ibc1 = fp32(1 / (1 - beta1^k))
//   u   = fma(wd_i, w, r)         when wd_i != 0, else r
//   phi_i = fdiv_rn(|w_i|, |u_i|) if adapt_i and both norms > 0, else 1; |x| = sqrt(S_x), the
//           root taken in double and rounded once to float
//   w'  = fma(-(lr_t * phi_i), u, w)         (lr_t * phi_i rounded once, negation exact)
// No clamp on |w| and no upper limit on phi.  The lines den .. u are lamb_u, the one function
// both kernels call on the same stored m', v' and the same w, so the u that pass 2 applies is
// bit for bit the u whose square pass 1 summed.  The TU is built without fast-math and every
// multiply-add pair is an explicit fmaf: contraction has nothing left to choose.
//
// Per-step scalars {ibc1, bc2_sqrt, lr_t, 0} come from a device-resident table (ops/lamb.py
// lamb_coef_table; float64 on the host, rounded once), entry min(t, n_coef - 1), t = sched->t
// (types.h SchedState).  Pass 1 reads t with sched_read_t and nothing else: it takes no ticket
// and does not advance t.  Pass 2 reads the same t, takes the tickets and calls sched_finish
// (the schedule protocol of flat_step.h), so the Adam step and the learning-rate schedule stay
// one counter.  A shadows-only pass 2 (a.update == 0) fills no table, reads no t and takes no
// ticket.
//
// Why pass 1 stores the moments.  Bytes of device memory traffic per element, counted:
//   this split: pass 1 reads w g m v (16), writes m' v' (8); pass 2 reads w m' v' (12),
//               writes w' (4) + bf16 shadow (2)                                          42
//   pass 1 only reduces (reads 16), pass 2 redoes the moment update
//               (reads 16, writes 12 + 2)                                                46
//   pass 1 writes a scratch copy of u (reads 16, writes 12), pass 2 reads w u (8),
//               writes 4 + 2: 42 too, plus a fifth parameter-sized buffer
//   adamw_kernel: reads 16, writes 12 + 2                                                30
// Storing m' and v' once is the cheapest split that keeps both passes' u identical without a
// fifth buffer; pass 2 never touches g.  u over the gradient buffer would also be 42 bytes, but
// the gradient is an input the step must not rewrite (accumulation, the clip's norm).
//
// lamb_moments_kernel - the work split and the summation are seg_sqnorm_kernel's (lars.hip
// header, steps 1 to 5), over the same LARS segment table: blocks of 256 threads, grid
// seg_sqnorm_blocks(n_items), block b takes items b, b + grid, ...; one item is at most 4096
// elements of one tensor; thread t owns quads q = j 256 + t, j = 0..3.  Per item:
//   - all 16 independent 16-byte loads (w, g, m, v quads) are issued before the first use,
//     through a clamped quad index; a thread whose quad lies past the item stores nothing and
//     contributes +0.0f;
//   - wd of the item's tensor is segs[item.seg].wd: one scalar load per item;
//   - per element m', v', u; m' and v' are stored.  An element at or past the item's len inside
//     the partial last quad is stored back unchanged and contributes +0.0f (dropped by a select:
//     NaN padding is never summed);
//   - 1. sq = fmaf(x, x, +0.0f) for x = w and x = u; 2. thread fold (a + b) + (c + d) per quad,
//     (s0 + s1) + (s2 + s3) per thread; 3. wave_sum; 4. ((w0 + w1) + w2) + w3 over the four waves
//     -> partials[e] = {w part, u part}, one 8-byte write-through store; 5. last_arrival
//     (relaxed ticket, agent-scope loads, no fence), then wave v takes tensors v, v + 4, ...,
//     lane j sums the item partials j, j + 64, ... sequentially from +0.0f, then wave_sum ->
//     sums[s] = {S_w, S_u}, trust[s] = {phi, wd, |w|, |u|} (seg_finish.h: one body for both kernels).
// S_w is therefore bit for bit seg_sqnorm_kernel's (kernel_bounds.replay_seg_sqnorm).  No float
// atomics, no agent-scope fence, no state across launches beyond the LARS workspace (partials,
// ticket, sums, trust) and SchedState.
//
// lamb_apply_kernel - LambRule on flat_stream: the m' buffer stands in the gradient's place
// (gs = 1, no CLIP build, as ema_kernel puts the parameters there) and the rule loads the v'
// quad itself.  {phi, wd} goes through LDS exactly as in lars_kernel: the cmap load depends on
// nothing and is issued with the quad's loads; the null segment {1, 0} serves padding chunks
// (w = m' = v' = 0 there: u = 0 and w stays 0).
#include "kernels/bn_tail.h"
#include "kernels/common.h"
#include "kernels/flat_step.h"
#include "kernels/launchers.h"
#include "kernels/seg_finish.h"

namespace ddp_amd {

// den, r and u of the definition; c = {ibc1, bc2_sqrt, lr_t, -}
__device__ __forceinline__ float lamb_u(float w, float m1, float v1, float wd, float ibc1, float bc2_sqrt,
                                        float eps) {
  const float den = __fadd_rn(sqrtf(v1) / bc2_sqrt, eps);
  const float r = __fmul_rn(m1 / den, ibc1);
  return wd != 0.f ? fmaf(wd, w, r) : r;
}

// One element of pass 1: the moment lines, then lamb_u.  live == false (at or past the item's
// len): the moments keep their values and both squares are +0.0f.
template <bool CLIP>
__device__ __forceinline__ void lamb_moment_one(float w, float d, float* m, float* v, bool live, const AdamArgs& a,
                                                float gs, float wd, const float4& c, float* sw, float* su) {
  if constexpr (CLIP) d = __fmul_rn(d, gs);
  if (a.maximize) d = -d;
  const float m1 = fmaf(a.w1, d - *m, *m);
  const float v1 = fmaf(a.w2 * d, d, a.b2 * (*v));
  const float u = lamb_u(w, m1, v1, wd, c.x, c.y, a.eps);
  *m = live ? m1 : *m;
  *v = live ? v1 : *v;
  *sw = live ? fmaf(w, w, 0.f) : 0.f;
  *su = live ? fmaf(u, u, 0.f) : 0.f;
}

template <bool CLIP>
__global__ __launch_bounds__(LARS_THREADS) void lamb_moments_kernel(
    const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mbuf, float* __restrict__ vbuf,
    long n, const LarsItem* __restrict__ items, int n_items, const LarsSeg* __restrict__ segs, int n_seg,
    float2* __restrict__ partials, int* __restrict__ ticket, float2* __restrict__ sums, float4* __restrict__ trust,
    AdamArgs a, const float* __restrict__ gscale, const float4* __restrict__ coef, int n_coef,
    const SchedState* __restrict__ sched) {
  static_assert(LARS_THREADS == 256 && LARS_ITEM == 4 * 4 * LARS_THREADS, "4 waves, 4 quads per thread and item");
  __shared__ float s_w[4], s_u[4];
  __shared__ int s_last;
  const int t = threadIdx.x;
  float gs = 1.f;
  if constexpr (CLIP) gs = gscale[0];
  const float4 c = coef[sched_index(sched_read_t(sched), n_coef)];  // read only: pass 2 advances t
  for (int e = blockIdx.x; e < n_items; e += gridDim.x) {
    const LarsItem it = items[e];
    long begin = (long)it.begin_chunk * LARS_CHUNK;
    int len = it.len;
    // (the host checked the table when it built it: an entry that does not fit the buffer is
    // summed as empty, never read or written)
    if (it.begin_chunk < 0 || len < 1 || len > LARS_ITEM || begin + ((len + 3) & ~3) > n || it.seg < 0 ||
        it.seg >= n_seg) { begin = 0; len = 0; }
    const float wd = segs[len > 0 ? it.seg : 0].wd;
    const int nq = (len + 3) >> 2;
    const float4* w4 = reinterpret_cast<const float4*>(w + begin);
    const float4* g4 = reinterpret_cast<const float4*>(g + begin);
    float4* m4 = reinterpret_cast<float4*>(mbuf + begin);
    float4* v4 = reinterpret_cast<float4*>(vbuf + begin);
    float4 xw[4], xg[4], xm[4], xv[4];
#pragma unroll
    // all sixteen loads issued before the first use; branch-free.  A thread whose quad lies past
    // the item reads the clamped quad nq - 1 of m and v, which its owner may already have
    // rewritten (unlike seg_sqnorm_kernel, this kernel stores): an unordered read, harmless
    // because such a thread drops every value by the selects below and stores nothing.
    for (int j = 0; j < 4; ++j) {
      const int q = j * LARS_THREADS + t;
      const int qi = q < nq ? q : (nq > 0 ? nq - 1 : 0);
      xw[j] = w4[qi];
      xg[j] = g4[qi];
      xm[j] = m4[qi];
      xv[j] = v4[qi];
    }
    float fw[4], fu[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = j * LARS_THREADS + t;
      const int left = len - 4 * q;  // elements of the item from this quad's first
      float aw, bw, cw, dw, au, bu, cu, du;
      lamb_moment_one<CLIP>(xw[j].x, xg[j].x, &xm[j].x, &xv[j].x, left > 0, a, gs, wd, c, &aw, &au);
      lamb_moment_one<CLIP>(xw[j].y, xg[j].y, &xm[j].y, &xv[j].y, left > 1, a, gs, wd, c, &bw, &bu);
      lamb_moment_one<CLIP>(xw[j].z, xg[j].z, &xm[j].z, &xv[j].z, left > 2, a, gs, wd, c, &cw, &cu);
      lamb_moment_one<CLIP>(xw[j].w, xg[j].w, &xm[j].w, &xv[j].w, left > 3, a, gs, wd, c, &dw, &du);
      fw[j] = (aw + bw) + (cw + dw);
      fu[j] = (au + bu) + (cu + du);
      if (q < nq) {  // a clamped quad belongs to another thread
        m4[q] = xm[j];
        v4[q] = xv[j];
      }
    }
    const float tw = wave_sum((fw[0] + fw[1]) + (fw[2] + fw[3]));
    const float tu = wave_sum((fu[0] + fu[1]) + (fu[2] + fu[3]));
    if ((t & 63) == 0) { s_w[t >> 6] = tw; s_u[t >> 6] = tu; }
    __syncthreads();
    if (t == 0)
      st_wt(partials + e, make_float2(((s_w[0] + s_w[1]) + s_w[2]) + s_w[3], ((s_u[0] + s_u[1]) + s_u[2]) + s_u[3]));
    __syncthreads();  // s_w / s_u are rewritten by the block's next item
  }
  if (!last_arrival(ticket, gridDim.x, &s_last)) return;

  seg_finish(segs, n_seg, n_items, partials, sums, trust, [](const LarsSeg& sg, float Sw, float Su) {
    const float wn = (float)sqrt((double)Sw);
    const float un = (float)sqrt((double)Su);
    const float phi = (sg.adapt && wn > 0.f && un > 0.f) ? __fdiv_rn(wn, un) : 1.f;
    return make_float4(phi, sg.wd, wn, un);
  });
}

void lamb_moments(const float* w, const float* g, float* mbuf, float* vbuf, long n, const LarsItem* items, int n_items,
                  const LarsSeg* segs, int n_seg, float* partials, int* ticket, float* sums, float* trust,
                  const AdamArgs& a, const float* gscale, const float* coef, int n_coef, const SchedState* sched,
                  hipStream_t s) {
  hipLaunchKernelGGL(gscale ? lamb_moments_kernel<true> : lamb_moments_kernel<false>,
                     dim3((unsigned)seg_sqnorm_blocks(n_items)), dim3(LARS_THREADS), 0, s, w, g, mbuf, vbuf, n, items,
                     n_items, segs, n_seg, reinterpret_cast<float2*>(partials), ticket, reinterpret_cast<float2*>(sums),
                     reinterpret_cast<float4*>(trust), a, gscale, reinterpret_cast<const float4*>(coef), n_coef, sched);
}

// lamb_apply_kernel's rule for flat_stream: v is w, d is m' (the buffer in the gradient's place);
// {phi, wd} = tab[min(cmap[i / 64], n_seg)] as LarsRule; c = {ibc1, bc2_sqrt, lr_t, -}
struct LambRule {
  const float* vbuf;
  float eps;
  float4 c;
  const short* cmap;
  const float2* tab;
  int n_seg;
  __device__ __forceinline__ unsigned seg(long i) const { return (unsigned)(int)cmap[i >> 6]; }
  __device__ __forceinline__ float2 entry(unsigned s) const { return tab[s < (unsigned)n_seg ? s : (unsigned)n_seg]; }
  __device__ __forceinline__ float apply(float w, float m1, float v1, const float2& pw) const {
    const float u = lamb_u(w, m1, v1, pw.y, c.x, c.y, eps);
    return fmaf(-__fmul_rn(c.z, pw.x), u, w);
  }
  __device__ __forceinline__ float4 quad(long q, float4 w, float4 m1) const {
    const unsigned s = seg(q << 2);
    const float4 v1 = reinterpret_cast<const float4*>(vbuf)[q];
    const float2 pw = entry(s);
    w.x = apply(w.x, m1.x, v1.x, pw);
    w.y = apply(w.y, m1.y, v1.y, pw);
    w.z = apply(w.z, m1.z, v1.z, pw);
    w.w = apply(w.w, m1.w, v1.w, pw);
    return w;
  }
  __device__ __forceinline__ float one(long i, float w, float m1) const {
    const unsigned s = seg(i);
    const float v1 = vbuf[i];
    return apply(w, m1, v1, entry(s));
  }
};

__global__ __launch_bounds__(FLAT_THREADS) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ mbuf,
    const float* __restrict__ vbuf, long n, AdamArgs a, ShadowSet sh, const short* __restrict__ cmap,
    const float4* __restrict__ trust, int n_seg, const float4* __restrict__ coef, int n_coef,
    SchedState* __restrict__ sched) {
  extern __shared__ float2 s_tab[];  // n_seg + 1 entries {phi, wd}; the last is the null segment
  int t = 0, ticket = -1;
  float4 c = {1.f, 1.f, 0.f, 0.f};
  if (a.update) {
    for (int i = threadIdx.x; i <= n_seg; i += blockDim.x) {
      const float4 r = trust[i];
      s_tab[i] = make_float2(r.x, r.y);
    }
    t = sched_read_t(sched);
    c = coef[sched_index(t, n_coef)];
    __syncthreads();  // the table is in LDS and every wave of the block has read t
    ticket = sched_ticket(sched);
  }
  flat_stream<false>(p, mbuf, n, a.update, 1.f, sh, LambRule{vbuf, a.eps, c, cmap, s_tab, n_seg});
  sched_finish(sched, t, ticket, c.z);
}

void lamb_step(float* p, const float* mbuf, const float* vbuf, long n, const AdamArgs& a, const ShadowSet& sh,
               const short* cmap, const float* trust, int n_seg, const float* coef, int n_coef, SchedState* sched,
               hipStream_t s) {
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(flat_grid(n)), dim3(FLAT_THREADS), (size_t)(n_seg + 1) * sizeof(float2), s,
                     p, mbuf, vbuf, n, a, sh, cmap, reinterpret_cast<const float4*>(trust), n_seg,
                     reinterpret_cast<const float4*>(coef), n_coef, sched);
}

}  // namespace ddp_amd
