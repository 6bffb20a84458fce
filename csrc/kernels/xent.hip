// Fused softmax cross-entropy forward + backward (reference train_ddp.py:40,198:
// nn.CrossEntropyLoss(), mean reduction).
//
// One workgroup of 4 waves; wave w owns rows b = w, w+4, ...; lane l owns
// classes c = l, l+64, ...  Per row: logits = bias + sum_g partials (fixed
// order: the split-K partial logits of the fc layer), max / sum-exp by wave
// butterflies, loss_b = logsumexp - logit[label],
// dlogits = (softmax - onehot) * gscale (gscale = 1/B for the mean).
// Also produces the fc bias gradient sum_b dlogits (prescaled for DDP) and the
// mean loss as a device scalar that the host reads only when it logs
// (every 100 batches, reference train_ddp.py:201-202).
// Labels come either from an int64 tensor or from the device-resident dataset
// labels through the epoch index list (BatchIdx).
// Wide heads take xent_wave_rows_kernel; both kernels evaluate one row body (xent_body.h).
#include "kernels/bn_tail.h"
#include "kernels/launchers.h"
#include "kernels/xent_body.h"

#include <stdexcept>
#include <string>

namespace ddp_amd {

static void xe_check(hipError_t e) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP: ") + hipGetErrorString(e));
}

// The row arithmetic and what SMOOTH / PAIR mean: xent_body.h.  This kernel's own part: the
// logits are the fixed-order sum of G partials plus the bias (with the optional logits_out
// store), only M = ceil(C / 64) steps are walked (10 classes: one), every dlogits element is
// also summed into dbias, each wave sums its rows' losses before the waves are summed; PAIR
// takes int64 labels only.
template <bool SMOOTH, bool PAIR>
__global__ __launch_bounds__(1024) void xent_kernel(const float* __restrict__ part, int G,
                                                   const float* __restrict__ bias, int C, int B,
                                                   const long long* __restrict__ labels64,
                                                   const int* __restrict__ labels32, BatchIdx bi,
                                                   float* __restrict__ logits_out,
                                                   float* __restrict__ dlogits,
                                                   float* __restrict__ loss_out,
                                                   float* __restrict__ dbias, float gscale,
                                                   float dbias_scale, XentSmooth<SMOOTH> sm,
                                                   XentPair<PAIR> pr) {
  __shared__ float s_loss[16];
  __shared__ float s_db[4][XENT_M * 64];  // dbias: 4 waves only (see xent())
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int M = (C + 63) / 64;
  float db[XENT_M];
#pragma unroll
  for (int m = 0; m < XENT_M; ++m) db[m] = 0.f;
  float lsum = 0.f;
  const int base = labels32 ? bi.base() : 0;
  for (int b = wave; b < B; b += nw) {
    const XentTarget t = xent_target(labels64 ? (int)labels64[b] : labels32[bi.row(b, base)], b, pr);
    float* const drow = dlogits + (long)b * C;
    float x[XENT_M];
    const XentRow r = xent_row_stats<SMOOTH, PAIR>(x, C, M, lane, t, [&](int c) {
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += part[((long)b * G + g) * C + c];
      const float v = s + (bias ? bias[c] : 0.f);
      if (logits_out) logits_out[(long)b * C + c] = v;
      return v;
    });
    lsum += xent_row_loss<SMOOTH, PAIR>(r, t, sm);
    xent_row_dlogits<SMOOTH, PAIR>(x, r, C, M, lane, t, sm, gscale, [&](int m, int c, float d) {
      drow[c] = d;
      if constexpr (SMOOTH) {
#pragma clang fp contract(off)  // dbias: the in-order sum of the stored dlogits, bit for bit
        db[m] += d;
      } else {
        db[m] += d;
      }
    });
  }
  if (lane == 0) s_loss[wave] = lsum;
  if (dbias) {
#pragma unroll
    for (int m = 0; m < XENT_M; ++m)
      if (m < M) s_db[wave][lane + 64 * m] = db[m];
  }
  __syncthreads();
  // graph-replayed steps log their loss into a per-epoch history indexed by the step counter
  if (threadIdx.x == 0 && loss_out) {
    float t = s_loss[0];
    for (int w = 1; w < nw; ++w) t += s_loss[w];
    loss_out[bi.step_ctr ? *bi.step_ctr : 0] = t / (float)B;
  }
  if (dbias)
    for (int c = threadIdx.x; c < C; c += 256)
      dbias[c] = (((s_db[0][c] + s_db[1][c]) + s_db[2][c]) + s_db[3][c]) * dbias_scale;
}

// Wide heads (64 < C <= 1024) over [B][C] fp32 logits: one wave per row (4 rows per block, B/4
// blocks) instead of one block looping over the rows, a logit one global read, always XENT_M
// steps.  Per-row losses go out write-through; the last block sums them in row order.
template <bool SMOOTH, bool PAIR>
__global__ __launch_bounds__(256) void xent_wave_rows_kernel(const float* __restrict__ logits, int C,
                                                             int B, const long long* __restrict__ labels,
                                                             float* __restrict__ dlogits,
                                                             float* __restrict__ loss_out,
                                                             float* __restrict__ ws, int* __restrict__ ticket,
                                                             float gscale, XentSmooth<SMOOTH> sm,
                                                             XentPair<PAIR> pr) {
  __shared__ int s_last;
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b < B) {
    const XentTarget t = xent_target((int)labels[b], b, pr);
    const float* const row = logits + (long)b * C;
    float* const drow = dlogits + (long)b * C;
    float x[XENT_M];
    const XentRow r = xent_row_stats<SMOOTH, PAIR>(x, C, XENT_M, lane, t, [&](int c) { return row[c]; });
    xent_row_dlogits<SMOOTH, PAIR>(x, r, C, XENT_M, lane, t, sm, gscale, [&](int, int c, float d) { drow[c] = d; });
    const float loss = xent_row_loss<SMOOTH, PAIR>(r, t, sm);
    if (lane == 0) st_wt(ws + b, loss);
  }
  if (!last_arrival(ticket, gridDim.x, &s_last)) return;
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int r = 0; r < B; ++r) t += ld_agent(ws + r);
    loss_out[0] = t / (float)B;
  }
}

// Engine variant (fusion level 0): one workgroup over the per-block partial logits
// [blk][2][NO] written by the fused conv2 epilogue, see xent_batch_block (xent_body.h).
// Writes per-row loss and dlogits; the batch mean loss and the fc bias gradient are
// finished by fc_bwd's first block (it holds dlogits).
__global__ __launch_bounds__(1024) void xent_rows_kernel(const float* __restrict__ part, int HW, int CH,
                                                        const float* __restrict__ bias, int NO,
                                                        int B, const int* __restrict__ labels32,
                                                        BatchIdx bi, float* __restrict__ dlogits,
                                                        float* __restrict__ loss_rows,
                                                        float gscale) {
  extern __shared__ float s_lg[];  // [B][NO] logits, then [B] labels
  xent_batch_block(part, HW, CH, bias, NO, B, labels32, bi, gscale, dlogits, loss_rows, s_lg,
                   reinterpret_cast<int*>(s_lg + B * NO));
}

void xent_rows(const float* part, int HW, int CH, const float* bias, int NO, int B,
               const int* labels32, BatchIdx bi, float* dlogits, float* loss_rows, float gscale,
               hipStream_t s) {
  const int threads = B * NO <= 256 ? 256 : (B * NO <= 512 ? 512 : 1024);
  hipLaunchKernelGGL(xent_rows_kernel, dim3(1), dim3(threads), sizeof(float) * B * (NO + 1), s, part, HW, CH,
                     bias, NO, B, labels32, bi, dlogits, loss_rows, gscale);
}

// Hands launch(sm, pr) the by-value arguments of one of the four builds: label_smoothing == 0
// the build without smoothing, no pair targets the build without them (the kernels as they
// always were).  keep and eps_c are each rounded once, here.
template <typename F>
static void xent_select_build(float label_smoothing, int C, const long long* labels_b, const float* pair_w,
                              F launch) {
  const XentSmooth<true> sm{1.f - label_smoothing, label_smoothing / (float)C};
  const XentPair<true> pr{labels_b, pair_w};
  const bool pair = labels_b && pair_w;
  if (label_smoothing != 0.f) {
    if (pair) launch(sm, pr);
    else launch(sm, XentPair<false>{});
  } else {
    if (pair) launch(XentSmooth<false>{}, pr);
    else launch(XentSmooth<false>{}, XentPair<false>{});
  }
}

// ResNet-width heads (C > 64, labels64, no bias fold): one wave per row; false if unsupported
static bool xent_wave_rows(const float* logits, int C, int B, const long long* labels, float* dlogits,
                           float* loss_out, float gscale, hipStream_t s, float label_smoothing,
                           const long long* labels_b, const float* pair_w) {
  constexpr int kMaxB = 8192;
  if (C > 64 * XENT_M || B > kMaxB || B < 1) return false;
  static float* wsp[64] = {};
  int dev = 0;
  xe_check(hipGetDevice(&dev));
  dev &= 63;
  if (!wsp[dev]) xe_check(hipMalloc(reinterpret_cast<void**>(&wsp[dev]), sizeof(float) * kMaxB));
  xent_select_build(label_smoothing, C, labels_b, pair_w, [&](auto sm, auto pr) {
    hipLaunchKernelGGL((xent_wave_rows_kernel<decltype(sm)::on, decltype(pr)::on>), dim3((B + 3) / 4), dim3(256), 0,
                       s, logits, C, B, labels, dlogits, loss_out, wsp[dev], bn_ticket_slots(1), gscale, sm, pr);
  });
  return true;
}

void xent(const float* part, int G, const float* bias, int C, int B, const long long* labels64,
          const int* labels32, BatchIdx bi, float* logits_out, float* dlogits, float* loss_out,
          float* dbias, float gscale, float dbias_scale, hipStream_t s, float label_smoothing,
          const long long* labels_b, const float* pair_w) {
  const bool pair = labels_b || pair_w;
  if (pair && !(labels_b && pair_w && labels64))
    throw std::invalid_argument("xent: pair targets need labels_b, pair_w and int64 labels (the fused engine's "
                                "labels32 / BatchIdx label source has no pair build)");
  // one wave per row when there is no bias gradient to fold (it is reduced over 4 waves)
  if (G == 1 && !bias && !dbias && !logits_out && labels64 && !bi.step_ctr && C > 64 &&
      xent_wave_rows(part, C, B, labels64, dlogits, loss_out, gscale, s, label_smoothing, labels_b, pair_w))
    return;
  const int waves = dbias ? 4 : (B < 16 ? (B < 4 ? 4 : B) : 16);
  xent_select_build(label_smoothing, C, labels_b, pair_w, [&](auto sm, auto pr) {
    hipLaunchKernelGGL((xent_kernel<decltype(sm)::on, decltype(pr)::on>), dim3(1), dim3(64 * waves), 0, s, part, G,
                       bias, C, B, labels64, labels32, bi, logits_out, dlogits, loss_out, dbias, gscale,
                       dbias_scale, sm, pr);
  });
}

DDP_STAMPS_SETTER(stamps_set_xent)

}  // namespace ddp_amd
