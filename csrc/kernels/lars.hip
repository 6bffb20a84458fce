// Flat-buffer LARS (layer-wise adaptive rate scaling): SGD with momentum in which every
// tensor's decayed gradient is first scaled by that tensor's trust ratio.  Two launches per
// step, both replayable by a captured graph: seg_sqnorm_kernel leaves every tensor's weight
// norm, gradient norm and trust ratio in device memory, and lars_kernel<CLIP, DLR> - the
// streaming pass of flat_step.h (flat_stream, shared with sgd_kernel and adamw_kernel), shadow
// refresh included - reads them there.
//
// The segment table (ops/lars.py lars_layout; a function of the parameter shapes alone, so
// the same on every GPU; every tensor begins on a 64-element boundary of the flat buffer):
//   segs[s]  = {begin / 64, numel, item0, n_items, wd, adapt, -, -}   one per tensor
//   items[e] = {begin / 64, len, s, k}: tensor s cut into pieces of LARS_ITEM = 4096 elements
//              (the last one shorter), in order; item0[s] + k = e; an item never spans tensors
//   cmap[c]  = the tensor that owns the 64-element chunk c, or n_seg (the null segment: ratio
//              1, wd 0) for a chunk that is padding only
//
// seg_sqnorm_kernel - exact order of the float operations (ops/kernel_bounds.py
// replay_seg_sqnorm replays it in numpy; the tests compare bit for bit).  Blocks of 256
// threads, grid min(n_items, LARS_MAX_BLOCKS); block b takes items b, b + grid, ...; for one
// item and each of the two buffers x = w and x = g alike:
//   1. Thread t owns quads q = u 256 + t, u = 0..3, of the item (elements 4 q + c, c = 0..3);
//      sq[u][c] = fmaf(x, x, +0.0f) (one rounding; an explicit fma, so the compiler's
//      contraction has nothing to fuse into step 2), +0.0f for an element at or past len (it is
//      loaded through a clamped index and dropped by a select: NaN padding is never summed).
//   2. Thread fold: s_u = (sq[u][0] + sq[u][1]) + (sq[u][2] + sq[u][3]), then
//      th = (s_0 + s_1) + (s_2 + s_3).
//   3. Wave: wave_sum (common.h), the balanced pairwise tree over lanes 0..63 (6 levels).
//   4. Block: ((w0 + w1) + w2) + w3 over its four waves -> partials[e] = {w part, g part}
//      (one 8-byte write-through store).
//   5. The block that arrives last (bn_tail.h last_arrival: relaxed ticket, partials read
//      with agent-scope loads, no fence): wave v takes tensors v, v + 4, ...; lane j sums
//      the tensor's item partials j, j + 64, j + 128, ... sequentially from +0.0f, then
//      step 3 gives S_w and S_g -> sums[s].
//   6. wn = sqrt(S_w), gn = sqrt(S_g), each correctly rounded (the root taken in double and
//      rounded to float, as grad_sqnorm_kernel); with clipping gn = gn * coef (one rounding,
//      coef = ClipStats::coef that grad_sqnorm_kernel left on the same stream);
//      ratio = fdiv_rn(trust_coef * wn, fmaf(wd, wn, gn) + eps) (product, fma, add, divide:
//      four roundings) if adapt and wn > 0 and gn > 0, else 1 -> trust[s] = {ratio, wd, wn, gn}.
// Longest chain of roundings into S: 1 + 2 + 2 + 6 + 3 + ceil(n_items / 64) + 6
// (kernel_bounds.seg_sqnorm_chain).  In flight per thread and item: 4 + 4 independent
// 16-byte loads, all issued before the first use (the clamp-and-zero form of grad_norm.hip).
//
// lars_kernel - geometry, the CLIP multiply and the schedule protocol: flat_step.h.
// A quad lies in one 64-element chunk, so in one tensor: s = cmap[i / 64], {ratio, wd} =
// trust[s].  Per element, all fp32, every line one rounding:
//   d = g                    CLIP: d = g * gscale[0]; maximize: d = -d (exact)
//   d = fmaf(wd, w, d)       when wd != 0
//   d = d * ratio
//   buf = d on the first step, else fmaf(1 - dampening, d, momentum * buf)   (momentum != 0;
//   d = fmaf(momentum, buf, d) with nesterov, else buf)                      sgd_one's lines)
//   w = fmaf(-lr, d, w)
// With ratio = 1 the product is exact and the sequence is sgd_one's, bit for bit.  DLR: lr is
// lr_table[min(t, n_table - 1)], t = sched->t, advanced inside the launch; a shadows-only
// launch (a.update == 0) is no optimizer step: it fills no table, reads no t and takes no
// ticket (as adamw_kernel; sgd_kernel<.., true> differs).
//
// The {ratio, wd} table goes through LDS: each block copies the n_seg + 1 entries (8 bytes
// each, at most 32 KiB) before its barrier.  Read straight from L2 the lookup would be two
// dependent loads (cmap, then trust) in front of every quad's arithmetic; with the copy the
// cmap load depends on nothing and is issued with the quad's p / g / momentum loads, and the
// dependent read is an LDS access.  The fill runs whenever a.update is set, with or without
// DLR, in front of the barrier the schedule protocol needs anyway.
#include "kernels/bn_tail.h"
#include "kernels/common.h"
#include "kernels/flat_step.h"
#include "kernels/launchers.h"

namespace ddp_amd {

int seg_sqnorm_blocks(int n_items) {
  return n_items < 1 ? 1 : (n_items > LARS_MAX_BLOCKS ? LARS_MAX_BLOCKS : n_items);
}

__device__ __forceinline__ float2 ld_agent2(const float2* p) {
  const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p),
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_float2(__uint_as_float((unsigned)v), __uint_as_float((unsigned)(v >> 32)));
}

// steps 1 and 2 for one quad: the squares of the elements below `left` (elements left in the
// item from this quad's first), folded
__device__ __forceinline__ float lars_sq4(float4 x, int left) {
  const float a = left > 0 ? fmaf(x.x, x.x, 0.f) : 0.f;
  const float b = left > 1 ? fmaf(x.y, x.y, 0.f) : 0.f;
  const float c = left > 2 ? fmaf(x.z, x.z, 0.f) : 0.f;
  const float d = left > 3 ? fmaf(x.w, x.w, 0.f) : 0.f;
  return (a + b) + (c + d);
}

__global__ __launch_bounds__(LARS_THREADS) void seg_sqnorm_kernel(
    const float* __restrict__ w, const float* __restrict__ g, long n, const LarsItem* __restrict__ items,
    int n_items, const LarsSeg* __restrict__ segs, int n_seg, float2* __restrict__ partials,
    int* __restrict__ ticket, float2* __restrict__ sums, float4* __restrict__ trust, float trust_coef,
    float eps, const float* __restrict__ gscale) {
  static_assert(LARS_THREADS == 256 && LARS_ITEM == 4 * 4 * LARS_THREADS, "4 waves, 4 quads per thread and item");
  __shared__ float s_w[4], s_g[4];
  __shared__ int s_last;
  const int t = threadIdx.x;
  for (int e = blockIdx.x; e < n_items; e += gridDim.x) {
    const LarsItem it = items[e];
    long begin = (long)it.begin_chunk * LARS_CHUNK;
    int len = it.len;
    // (the host checked the table when it built it: an entry that does not fit the buffer is
    // summed as empty, never read)
    if (it.begin_chunk < 0 || len < 1 || len > LARS_ITEM || begin + ((len + 3) & ~3) > n) { begin = 0; len = 0; }
    const int nq = (len + 3) >> 2;
    const float4* w4 = reinterpret_cast<const float4*>(w + begin);
    const float4* g4 = reinterpret_cast<const float4*>(g + begin);
    float4 vw[4], vg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // all eight loads issued before the first use; branch-free
      const int q = u * LARS_THREADS + t;
      const int qi = q < nq ? q : (nq > 0 ? nq - 1 : 0);
      vw[u] = w4[qi];
      vg[u] = g4[qi];
    }
    float sw[4], sg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int left = len - 4 * (u * LARS_THREADS + t);
      sw[u] = lars_sq4(vw[u], left);
      sg[u] = lars_sq4(vg[u], left);
    }
    const float tw = wave_sum((sw[0] + sw[1]) + (sw[2] + sw[3]));
    const float tg = wave_sum((sg[0] + sg[1]) + (sg[2] + sg[3]));
    if ((t & 63) == 0) { s_w[t >> 6] = tw; s_g[t >> 6] = tg; }
    __syncthreads();
    if (t == 0)
      st_wt(partials + e, make_float2(((s_w[0] + s_w[1]) + s_w[2]) + s_w[3], ((s_g[0] + s_g[1]) + s_g[2]) + s_g[3]));
    __syncthreads();  // s_w / s_g are rewritten by the block's next item
  }
  if (!last_arrival(ticket, gridDim.x, &s_last)) return;

  const int wave = t >> 6, lane = t & 63;
  const float coef = gscale ? gscale[0] : 1.f;
  for (int s = wave; s < n_seg; s += 4) {
    const LarsSeg sg = segs[s];
    int ni = sg.n_items;
    if (sg.item0 < 0 || ni < 0 || (long)sg.item0 + ni > n_items) ni = 0;
    float aw = 0.f, ag = 0.f;
    for (int k = lane; k < ni; k += 64) {
      const float2 p = ld_agent2(partials + sg.item0 + k);
      aw += p.x;
      ag += p.y;
    }
    const float Sw = wave_sum(aw), Sg = wave_sum(ag);
    if (lane == 0) {
      const float wn = (float)sqrt((double)Sw);
      float gn = (float)sqrt((double)Sg);
      if (gscale) gn = __fmul_rn(gn, coef);
      float ratio = 1.f;
      if (sg.adapt && wn > 0.f && gn > 0.f)
        ratio = __fdiv_rn(__fmul_rn(trust_coef, wn), __fadd_rn(fmaf(sg.wd, wn, gn), eps));
      sums[s] = make_float2(Sw, Sg);
      trust[s] = make_float4(ratio, sg.wd, wn, gn);
    }
  }
}

void seg_sqnorm(const float* w, const float* g, long n, const LarsItem* items, int n_items, const LarsSeg* segs,
                int n_seg, float* partials, int* ticket, float* sums, float* trust, float trust_coef, float eps,
                const float* gscale, hipStream_t s) {
  hipLaunchKernelGGL(seg_sqnorm_kernel, dim3((unsigned)seg_sqnorm_blocks(n_items)), dim3(LARS_THREADS), 0, s, w, g,
                     n, items, n_items, segs, n_seg, reinterpret_cast<float2*>(partials), ticket,
                     reinterpret_cast<float2*>(sums), reinterpret_cast<float4*>(trust), trust_coef, eps, gscale);
}

// rw = {ratio, wd} of the element's tensor; a.weight_decay is not read
__device__ __forceinline__ float lars_one(float v, float d, float* mb, const SgdArgs& a, const float2& rw) {
  if (a.maximize) d = -d;
  if (rw.y != 0.f) d = fmaf(rw.y, v, d);
  d = __fmul_rn(d, rw.x);
  if (a.momentum != 0.f) {
    const float buf = a.first_step ? d : fmaf(1.f - a.dampening, d, a.momentum * (*mb));
    *mb = buf;
    d = a.nesterov ? fmaf(a.momentum, buf, d) : buf;
  }
  return fmaf(-a.lr, d, v);
}

// lars_kernel's rule for flat_stream: lars_one with the {ratio, wd} of the quad's tensor,
// tab[min(cmap[i / 64], n_seg)] (n_seg: the null segment; the host sized cmap to ceil(n / 64))
struct LarsRule {
  float* mbuf;
  SgdArgs a;
  const short* cmap;
  const float2* tab;
  int n_seg;
  // the tensor of flat element i: a load that depends on nothing - issue it with the quad's
  // other loads, before entry() (the dependent LDS read) waits for it
  __device__ __forceinline__ unsigned seg(long i) const { return (unsigned)(int)cmap[i >> 6]; }
  __device__ __forceinline__ float2 entry(unsigned s) const { return tab[s < (unsigned)n_seg ? s : (unsigned)n_seg]; }
  __device__ __forceinline__ float4 quad(long q, float4 v, float4 d) const {
    const unsigned s = seg(q << 2);
    float4 m = {0.f, 0.f, 0.f, 0.f};
    if (a.momentum != 0.f) m = reinterpret_cast<const float4*>(mbuf)[q];
    const float2 rw = entry(s);
    v.x = lars_one(v.x, d.x, &m.x, a, rw);
    v.y = lars_one(v.y, d.y, &m.y, a, rw);
    v.z = lars_one(v.z, d.z, &m.z, a, rw);
    v.w = lars_one(v.w, d.w, &m.w, a, rw);
    if (a.momentum != 0.f) reinterpret_cast<float4*>(mbuf)[q] = m;
    return v;
  }
  __device__ __forceinline__ float one(long i, float v, float d) const {
    const unsigned s = seg(i);
    float m = (a.momentum != 0.f) ? mbuf[i] : 0.f;
    v = lars_one(v, d, &m, a, entry(s));
    if (a.momentum != 0.f) mbuf[i] = m;
    return v;
  }
};

template <bool CLIP, bool DLR>
__global__ __launch_bounds__(FLAT_THREADS) void lars_kernel(float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ mbuf, long n, SgdArgs a, ShadowSet sh, const short* __restrict__ cmap,
    const float4* __restrict__ trust, int n_seg, const float* __restrict__ gscale, const float* __restrict__ lr_table,
    int n_table, SchedState* __restrict__ sched) {
  extern __shared__ float2 s_tab[];  // n_seg + 1 entries {ratio, wd}; the last is the null segment
  float gs = 1.f;
  if constexpr (CLIP) gs = gscale[0];
  int t = 0, ticket = -1;
  if (a.update) {
    for (int i = threadIdx.x; i <= n_seg; i += blockDim.x) {
      const float4 r = trust[i];
      s_tab[i] = make_float2(r.x, r.y);
    }
    if constexpr (DLR) {
      t = sched_read_t(sched);
      a.lr = lr_table[sched_index(t, n_table)];
    }
    __syncthreads();  // the table is in LDS; DLR: every wave of the block has read t
    if constexpr (DLR) ticket = sched_ticket(sched);
  }
  flat_stream<CLIP>(p, g, n, a.update, gs, sh, LarsRule{mbuf, a, cmap, s_tab, n_seg});
  if constexpr (DLR) sched_finish(sched, t, ticket, a.lr);
}

void lars_step(float* p, const float* g, float* mbuf, long n, const SgdArgs& a, const ShadowSet& sh,
               const short* cmap, const float* trust, int n_seg, hipStream_t s, const float* gscale,
               const float* lr_table, int n_table, SchedState* sched) {
  const bool dlr = sched != nullptr && lr_table != nullptr && n_table > 0;
  auto kernel = gscale ? (dlr ? lars_kernel<true, true> : lars_kernel<true, false>)
                       : (dlr ? lars_kernel<false, true> : lars_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(flat_grid(n)), dim3(FLAT_THREADS), (size_t)(n_seg + 1) * sizeof(float2), s, p, g, mbuf, n, a,
                     sh, cmap, reinterpret_cast<const float4*>(trust), n_seg, gscale, lr_table, n_table, sched);
}

}  // namespace ddp_amd
