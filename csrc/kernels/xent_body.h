// Device bodies of the softmax cross-entropy kernels, each piece of arithmetic written once: the
// SimpleCNN engine's thread-per-logit body (below), and first the wave-per-row body of
// xent_kernel and xent_wave_rows_kernel (xent.hip): lane l owns classes c = l, l + 64, ... (step
// m: c = l + 64 m, at most XENT_M steps = 1024 classes).  Per row: max / sum-exp by wave
// butterflies, loss_b = logsumexp - logit[label], dlogits = (softmax - onehot) * gscale.  What
// differs between the kernels - where a logit comes from, where a dlogits element goes, how many
// steps there are, how the row losses are summed - comes in from the caller as a functor or a
// value; nothing here asks who calls.
// SMOOTH: label smoothing as torch's (the mass eps goes over all C classes, the true one
// included): target = keep * onehot + eps_c, keep = 1 - eps and eps_c = eps / C rounded once on
// the host and passed by value (a captured step replays them).  One more wave reduction per row,
// S = sum_c (x_c - mx) over the C valid classes (per lane in class order, then wave_sum: a fixed
// order), and one more subtraction per element; no extra memory traffic.
// PAIR: the row trains against wa * t(y_a) + wb * t(y_b) (mixup / cutmix; t the smoothed
// one-hot), y_b and (wa, wb) read from device memory.  k_c = wa [c == y_a] + wb [c == y_b] (both
// terms when y_a == y_b) replaces the one-hot: dlogits_c = ((p_c - keep k_c) - eps_c) gscale and
// loss = log(se) - [keep fmaf(wa, x_a - mx, wb (x_b - mx)) + eps_c S].  One more compare per
// element and one more wave reduction per row.
// SMOOTH = false / PAIR = false are the kernels as they were before either: their XentSmooth /
// XentPair is empty.  Labels are only compared against, never indexed with: a label outside
// [0, C) reads and writes nothing out of bounds.
#pragma once
#include "kernels/common.h"

namespace ddp_amd {

constexpr int XENT_M = 16;  // steps of 64 lanes: up to 1024 classes

struct XentTarget {  // the row's target: y_a, and under PAIR y_b with the two weights
  int label, label_b;
  float wa, wb;
};
template <bool PAIR>
__device__ __forceinline__ XentTarget xent_target(int label, int b, XentPair<PAIR> pr) {
  XentTarget t{label, -1, 1.f, 0.f};
  if constexpr (PAIR) {
    t.label_b = (int)pr.labels_b[b];
    t.wa = pr.w[2 * b];
    t.wb = pr.w[2 * b + 1];
  }
  return t;
}

// One row's reductions on every lane: max, sum-exp, logit[y_a], logit[y_b] (PAIR), S (SMOOTH).
struct XentRow {
  float mx, se, xl, xb, sx;
};
// ld(c): logit c of the row, called once per valid class in step order.  M: the steps to walk
// (a constant XENT_M folds the tests on it away).  Leaves x[m] = exp(x_c - mx), 0 past C.
template <bool SMOOTH, bool PAIR, typename Ld>
__device__ __forceinline__ XentRow xent_row_stats(float (&x)[XENT_M], int C, int M, int lane, const XentTarget& t,
                                                  Ld ld) {
  XentRow r{-INFINITY, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < XENT_M; ++m) {
    if (m >= M) break;
    const int c = lane + 64 * m;
    x[m] = c < C ? ld(c) : -INFINITY;
    r.mx = fmaxf(r.mx, x[m]);
  }
  r.mx = wave_max(r.mx);
#pragma unroll
  for (int m = 0; m < XENT_M; ++m) {
    if (m >= M) break;
    const int c = lane + 64 * m;
    if (c == t.label) r.xl = x[m];
    if constexpr (PAIR) {
      if (c == t.label_b) r.xb = x[m];
    }
    if constexpr (SMOOTH) {
      if (c < C) r.sx += x[m] - r.mx;  // lanes / steps past C add exactly 0, not -inf
    }
    x[m] = c < C ? __expf(x[m] - r.mx) : 0.f;
    r.se += x[m];
  }
  r.se = wave_sum(r.se);
  r.xl = wave_sum(r.xl);                        // logit[label]
  if constexpr (PAIR) r.xb = wave_sum(r.xb);    // logit[label_b]
  if constexpr (SMOOTH) r.sx = wave_sum(r.sx);  // S = sum_c (x_c - mx)
  return r;
}

// The PAIR cross-entropy builds' target share of one class: keep * (ka + kb) (keep only with
// smoothing), ka / kb the row's two weights where the class is y_a / y_b and 0 elsewhere.
// Each operation rounds on its own (nothing contracts into the caller's subtraction), so
// ka = 1, kb = 0 gives exactly the keep / 1 the builds without pair targets subtract.
template <bool SMOOTH>
__device__ __forceinline__ float xent_pair_share(float ka, float kb, XentSmooth<SMOOTH> sm) {
#pragma clang fp contract(off)
  const float k = ka + kb;
  if constexpr (SMOOTH) return sm.keep * k;
  else return k;
}
// The target's share k of class c (without the eps_c every class gets); p - k has one form in
// every build.
template <bool SMOOTH, bool PAIR>
__device__ __forceinline__ float xent_share(int c, const XentTarget& t, XentSmooth<SMOOTH> sm) {
  if constexpr (PAIR) return xent_pair_share(c == t.label ? t.wa : 0.f, c == t.label_b ? t.wb : 0.f, sm);
  else if constexpr (SMOOTH) return c == t.label ? sm.keep : 0.f;
  else return c == t.label ? 1.f : 0.f;
}
// One dlogits element from the class's exponential e and share k.
template <bool SMOOTH>
__device__ __forceinline__ float xent_dlogit(float e, float inv, float k, XentSmooth<SMOOTH> sm, float gscale) {
  if constexpr (SMOOTH) return ((e * inv - k) - sm.eps_c) * gscale;
  else return (e * inv - k) * gscale;
}
// The row's dlogits; st(m, c, d) takes element c (step m) - every valid class once, in step order.
template <bool SMOOTH, bool PAIR, typename St>
__device__ __forceinline__ void xent_row_dlogits(const float (&x)[XENT_M], const XentRow& r, int C, int M, int lane,
                                                 const XentTarget& t, XentSmooth<SMOOTH> sm, float gscale, St st) {
  const float inv = 1.f / r.se;
#pragma unroll
  for (int m = 0; m < XENT_M; ++m) {
    if (m >= M) break;
    const int c = lane + 64 * m;
    const float k = xent_share<SMOOTH, PAIR>(c, t, sm);
    if (c < C) st(m, c, xent_dlogit(x[m], inv, k, sm, gscale));
  }
}
template <bool SMOOTH, bool PAIR>
__device__ __forceinline__ float xent_row_loss(const XentRow& r, const XentTarget& t, XentSmooth<SMOOTH> sm) {
  // log(se) - (xl - mx), not (mx + log(se)) - xl: the latter rounds at the logits' own
  // magnitude (an offset of 1e4 costs 5e-4 of the row's loss), xl - mx is (nearly) exact
  float zt = r.xl - r.mx;  // the target's logit relative to the row maximum
  if constexpr (PAIR) zt = fmaf(t.wa, r.xl - r.mx, t.wb * (r.xb - r.mx));
  // SMOOTH: log(se) - [keep (xl - mx) + eps_c S], every term relative to the row maximum, as above
  if constexpr (SMOOTH) return __logf(r.se) - fmaf(sm.eps_c, r.sx, sm.keep * zt);
  else return __logf(r.se) - zt;
}

// ---------------------------------------------------------------- SimpleCNN engine
// Whole-batch softmax cross-entropy on one workgroup, fixed summation order.
// part: the fused conv2+fc epilogue's partial logits, one pair of [NO] rows per conv
// block of CH consecutive pixels of the flattened [B*HW] space: part[blk][slot][o],
// slot 0 = the image of the block's first pixel, slot 1 = the next image (CH <= HW).
// Image b's logits are the fixed-order sum over the blocks kb0..kb1 that touch it.
// Phase 0: thread b < B requests its row's label (a dependent step -> index -> label
// chain) before anything else.  Phase 1: one thread per logit (b, o) loads its <= 16
// block partials (clamped block index, masked) and adds the bias -> s_lg[b][o] (LDS
// scratch, B*NO floats; the prefetched labels go to s_lab, B ints).  Phase 2: one thread
// per logit again; each evaluates its row's max / sum-exp serially over the NO classes
// (same order in every thread of the row, so bit-identical) and then its own class.
// Writes dl[b*NO + o] = (softmax - onehot) * gscale and loss[b] = logsumexp - x[label].  Contains a __syncthreads(): every thread of the
// block must call it; dl / loss may be LDS or global, and the caller syncs before
// reading them.  Used by xent_rows (own kernel) and by the XENT prologue of fc_bwd, so
// both produce bit-identical values.
constexpr int XENT_MAX_BLK = 16;  // conv blocks per image: HW / CH + 2 <= 16
// The fc_bwd prologue's variant: the whole partial array (nblk * 2 * NO floats, 15.7 KB
// at B = 32) is copied to LDS with coalesced 16-byte loads issued FIRST in the kernel,
// then every logit sums its partials from LDS in the same fixed order.  (Per-logit
// global loads are 16 scattered 4-byte loads per thread: ~5k lane-addresses per block
// through the texture addresser, measured ~2 us.)
constexpr int XENT_PRE_Q = 4;  // float4 per thread held from the prefetch to the LDS write
// The two fixed-order pieces every producer of dL shares (xent_finish below, the fc_bwd
// prologue, and the level-3 conv forward that computes dZ2 itself): one inlined body each,
// so every caller evaluates the same float operations in the same order (bit-identical).
// Image b's raw logit o (before the bias): sum over the conv blocks kb0..kb1 touching it of
// part[kb][slot][o] (slot 1 only for a first block that started in the previous image).
// The index sequence of that sum: term j (0 <= j < XENT_MAX_BLK) reads part[xent_logit_idx]
// (block index clamped to kb1; the clamped terms are added as +0.0f).
__device__ __forceinline__ int xent_logit_idx(int b, int o, int HW, int CH, int NO, int j) {
  const int p0 = b * HW;
  const int kb0 = p0 / CH, kb1 = (p0 + HW - 1) / CH;
  const int slot0 = kb0 * CH == p0 ? 0 : 1;
  const int kb = min(kb0 + j, kb1);
  return (kb * 2 + (j == 0 ? slot0 : 0)) * NO + o;
}
// Terms [J0, J1) of the sum added to a, j ascending; ld(j, i) returns term j's value part[i].
// The whole sum is the ranges chained in order from +0.0f (the level-3 forward sums the
// granules it swept in two halves; every other caller in one piece through xent_logit_acc).
template <int J0, int J1, typename Ld>
__device__ __forceinline__ float xent_logit_acc_range(float a, int b, int o, int HW, int CH, int NO, Ld ld) {
  const int p0 = b * HW;
  const int kb0 = p0 / CH, kb1 = (p0 + HW - 1) / CH;
#pragma unroll
  for (int j = J0; j < J1; ++j) {
    const float v = ld(j, xent_logit_idx(b, o, HW, CH, NO, j));
    a += (kb0 + j <= kb1) ? v : 0.f;
  }
  return a;
}
template <typename Ld>
__device__ __forceinline__ float xent_logit_acc(int b, int o, int HW, int CH, int NO, Ld ld) {
  return xent_logit_acc_range<0, XENT_MAX_BLK>(0.f, b, o, HW, CH, NO, [&](int, int i) { return ld(i); });
}
// dL[o] of one row x[0..NO) (softmax - onehot, times gscale); *loss (if o == 0 and loss)
// = logsumexp - x[label].  label is clamped to [0, NO).
__device__ __forceinline__ float xent_row_dl(const float* x, int NO, int o, int label, float gscale,
                                             float* loss) {
  label = label < 0 ? 0 : (label >= NO ? NO - 1 : label);
  float mx = x[0];
  for (int k = 1; k < NO; ++k) mx = fmaxf(mx, x[k]);
  float se = 0.f;
  for (int k = 0; k < NO; ++k) se += __expf(x[k] - mx);
  const float inv = 1.f / se;
  if (o == 0 && loss) *loss = mx + __logf(se) - x[label];
  return (__expf(x[o] - mx) * inv - (o == label ? 1.f : 0.f)) * gscale;
}
struct XentPre {
  int lab0;
  float bias_o;  // bias[threadIdx.x % NO]
  float4 q[XENT_PRE_Q];
};
__device__ __forceinline__ void xent_prefetch(const float* __restrict__ part, int npart,
                                              const float* __restrict__ bias, int NO, int B,
                                              const int* __restrict__ labels32, const BatchIdx& bi,
                                              XentPre& pre) {
  const float4* p4 = reinterpret_cast<const float4*>(part);
  const int n4 = npart >> 2;
#pragma unroll
  for (int k = 0; k < XENT_PRE_Q; ++k) {
    const int i = threadIdx.x + k * blockDim.x;
    pre.q[k] = i < n4 ? p4[i] : make_float4(0.f, 0.f, 0.f, 0.f);  // fully defined: stays in VGPRs
  }
  pre.lab0 = (int)threadIdx.x < B ? labels32[bi.row(threadIdx.x, bi.base())] : 0;
  pre.bias_o = (int)threadIdx.x < B * NO ? bias[threadIdx.x % NO] : 0.f;
  DDP_STAMP(STAMP_K_XENT, 1);  // loads issued
}
// s_part: npart floats of LDS (may alias scratch the caller uses only afterwards).
__device__ __forceinline__ void xent_finish(const XentPre& pre, const float* __restrict__ part, int npart,
                                            int HW, int CH, const float* __restrict__ bias, int NO, int B,
                                            const int* __restrict__ labels32, const BatchIdx& bi,
                                            float gscale, float* dl, float* loss, float* s_lg, int* s_lab,
                                            float* s_part) {
  const int n4 = npart >> 2;
  float4* s4 = reinterpret_cast<float4*>(s_part);
#pragma unroll
  for (int k = 0; k < XENT_PRE_Q; ++k) {
    const int i = threadIdx.x + k * blockDim.x;
    if (i < n4) s4[i] = pre.q[k];
  }
  for (int i = threadIdx.x + XENT_PRE_Q * blockDim.x; i < n4; i += blockDim.x)
    s4[i] = reinterpret_cast<const float4*>(part)[i];
  if ((int)threadIdx.x < B) s_lab[threadIdx.x] = pre.lab0;
  __syncthreads();
  DDP_STAMP(STAMP_K_XENT, 2);  // partials in LDS
  // the thread's first logit uses only prefetched / LDS operands; later logits (B * NO >
  // blockDim) run in a separate guarded loop - a global load the compiler may hoist into
  // the first iteration would wait (vmcnt in order) for all of the caller's column loads
  auto logit_sum = [&](int t) {
    const int b = t / NO, o = t - (t / NO) * NO;
    return xent_logit_acc(b, o, HW, CH, NO, [&](int i) { return s_part[i]; });
  };
  if ((int)threadIdx.x < B * NO) s_lg[threadIdx.x] = pre.bias_o + logit_sum(threadIdx.x);
  if (B * NO > (int)blockDim.x)
    for (int t = threadIdx.x + blockDim.x; t < B * NO; t += blockDim.x) s_lg[t] = bias[t % NO] + logit_sum(t);
  DDP_STAMP(STAMP_K_FC_BWD, 5);
  __syncthreads();
  DDP_STAMP(STAMP_K_FC_BWD, 6);
  auto row_out = [&](int t, int label) {
    const int b = t / NO, o = t - (t / NO) * NO;
    dl[t] = xent_row_dl(s_lg + b * NO, NO, o, label, gscale, loss + b);
  };
  // first logit: b = threadIdx.x / NO < blockDim, so its label is in s_lab (no pointer
  // select: the compiler would merge LDS / global into one flat load counted in vmcnt)
  if ((int)threadIdx.x < B * NO) row_out(threadIdx.x, s_lab[threadIdx.x / NO]);
  if (B * NO > (int)blockDim.x)
    for (int t = threadIdx.x + blockDim.x; t < B * NO; t += blockDim.x) {
      const int b = t / NO;
      row_out(t, b < (int)blockDim.x ? s_lab[b] : labels32[bi.row(b, bi.base())]);
    }
  DDP_STAMP(STAMP_K_FC_BWD, 7);
}
__device__ __forceinline__ void xent_batch_block(const float* __restrict__ part, int HW, int CH,
                                                 const float* __restrict__ bias, int NO, int B,
                                                 const int* __restrict__ labels32, const BatchIdx& bi,
                                                 float gscale, float* dl, float* loss, float* s_lg,
                                                 int* s_lab) {
  const int base = bi.base();
  const int lab0 = (int)threadIdx.x < B ? labels32[bi.row(threadIdx.x, base)] : 0;
  for (int t = threadIdx.x; t < B * NO; t += blockDim.x) {
    // 32-bit index math only (B * HW < 2^31, checked on the host): 64-bit divisions
    // by runtime values are long software sequences.  Block kb0 is the only one that can
    // start in the previous image (slot 1); every later block starts inside image b.
    const int b = t / NO, o = t - (t / NO) * NO;
    s_lg[t] = bias[o] + xent_logit_acc(b, o, HW, CH, NO, [&](int i) { return part[i]; });
  }
  if ((int)threadIdx.x < B) s_lab[threadIdx.x] = lab0;
  __syncthreads();
  // Phase 2, one thread per logit again: every thread of row b evaluates the row's max
  // and sum-exp in the same serial order (bit-identical values), then its own class.
  for (int t = threadIdx.x; t < B * NO; t += blockDim.x) {
    const int b = t / NO, o = t - (t / NO) * NO;
    const int label = b < (int)blockDim.x ? s_lab[b] : labels32[bi.row(b, base)];
    dl[t] = xent_row_dl(s_lg + b * NO, NO, o, label, gscale, loss + b);
  }
}

}  // namespace ddp_amd
