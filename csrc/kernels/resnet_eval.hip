// ResNet held-out evaluation: the folded BatchNorm vectors of the inference convolutions
// (conv_infer.h), the per-image tail behind the classifier head and the running totals.
//
// Tail: one wave per row of fp32 logits, like xent_wave_rows_kernel (xent.hip), but for any class
// count (the row is walked in 64-class steps, twice: maximum and label logit first, then
// the sum of exponentials, the lowest index of the maximum and the label's rank).
#include <stdexcept>

#include "kernels/common.h"
#include "kernels/conv_infer.h"

namespace ddp_amd {

__global__ __launch_bounds__(256) void bn_fold_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, int C,
                                                      float* __restrict__ sc, float* __restrict__ sh) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float invstd = rsqrtf(var[c] + eps);
  const float s = invstd * gamma[c];
  sc[c] = s;
  sh[c] = fmaf(-mean[c], s, beta[c]);  // bn_affine.h's definition
}

void bn_fold(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
             float eps, int C, float* sc, float* sh, hipStream_t s) {
  if (C <= 0) return;
  hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, s, running_mean, running_var, gamma,
                     beta, eps, C, sc, sh);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}

__global__ __launch_bounds__(256) void resnet_eval_tail_kernel(const float* __restrict__ logits, int C, int B,
                                                               const long long* __restrict__ labels,
                                                               int* __restrict__ pred, float* __restrict__ loss,
                                                               int* __restrict__ correct,
                                                               int* __restrict__ correct5) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform
  const float* row = logits + (long)b * C;
  const long long lab64 = labels[b];
  const int label = lab64 < 0 ? 0 : (lab64 >= C ? C - 1 : (int)lab64);  // (host validates; never out of bounds)
  const float xl = row[label];
  float mx = -INFINITY;
  int nan = 0;
  for (int c = lane; c < C; c += 64) {
    const float x = row[c];
    nan |= x != x;
    mx = fmaxf(mx, x);
  }
  mx = wave_max(mx);
  nan = wave_sum_i(nan);
  float se = 0.f;
  int first = C, before = 0;
  for (int c = lane; c < C; c += 64) {
    const float x = row[c];
    se += __expf(x - mx);
    if (x == mx) first = min(first, c);
    before += (x > xl || (x == xl && c < label)) ? 1 : 0;
  }
  se = wave_sum(se);
  first = wave_min_i(first);
  before = wave_sum_i(before);
  if (lane == 0) {
    // a NaN anywhere makes the row's maximum NaN (torch.max): no class equals it -> 0
    const int p = (nan || first >= C) ? 0 : first;
    pred[b] = p;
    // log(se) - (xl - mx), as xent_row_loss, xent_body.h (xl - mx is nearly exact)
    loss[b] = __logf(se) - (xl - mx);
    correct[b] = (long long)p == lab64 ? 1 : 0;
    correct5[b] = before < 5 ? 1 : 0;
  }
}

void resnet_eval_tail(const float* logits, int C, int B, const long long* labels, int* pred, float* loss,
                      int* correct, int* correct5, hipStream_t s) {
  if (!logits || !labels || !pred || !loss || !correct || !correct5)
    throw std::runtime_error("resnet_eval_tail: null buffer");
  if (C < 1) throw std::runtime_error("resnet_eval_tail: need at least one class");
  if (B <= 0) return;
  hipLaunchKernelGGL(resnet_eval_tail_kernel, dim3((B + 3) / 4), dim3(256), 0, s, logits, C, B, labels, pred, loss,
                     correct, correct5);
}

// One block, as infer_totals (infer.hip): the fp64 loss sum continues in INDEX order through
// every batch of a split, so the totals do not depend on the batching.
constexpr int RT_THREADS = 256, RT_CHUNK = 1024;
__global__ __launch_bounds__(RT_THREADS) void resnet_eval_totals_kernel(const int* __restrict__ correct,
                                                                        const int* __restrict__ correct5,
                                                                        const float* __restrict__ loss, int n,
                                                                        long long* __restrict__ tot,
                                                                        double* __restrict__ tot_loss) {
  __shared__ float s_loss[RT_CHUNK];
  __shared__ int s_ok[RT_CHUNK], s_ok5[RT_CHUNK];
  long long c = 0, c5 = 0;
  double l = 0.0;
  if (threadIdx.x == 0) { c = tot[0]; c5 = tot[1]; l = tot_loss[0]; }
  for (int i0 = 0; i0 < n; i0 += RT_CHUNK) {
    const int m = n - i0 < RT_CHUNK ? n - i0 : RT_CHUNK;
    for (int i = threadIdx.x; i < m; i += RT_THREADS) {
      s_loss[i] = loss[i0 + i];
      s_ok[i] = correct[i0 + i];
      s_ok5[i] = correct5[i0 + i];
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) {
        l += (double)s_loss[i];
        c += s_ok[i];
        c5 += s_ok5[i];
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) { tot[0] = c; tot[1] = c5; tot_loss[0] = l; }
}

void resnet_eval_totals(const int* correct, const int* correct5, const float* loss, int n, long long* tot,
                        double* tot_loss, hipStream_t s) {
  if (!correct || !correct5 || !loss || !tot || !tot_loss) throw std::runtime_error("resnet_eval_totals: null buffer");
  if (n <= 0) return;
  hipLaunchKernelGGL(resnet_eval_totals_kernel, dim3(1), dim3(RT_THREADS), 0, s, correct, correct5, loss, n, tot,
                     tot_loss);
}

}  // namespace ddp_amd
