// Inference entry points of the ResNet kernels (evaluation: frozen BatchNorm statistics).
// Kept out of launchers.h so that the TUs which only include that header do not rebuild.
//
// With running statistics BatchNorm is a per-channel affine, so it rides in the
// convolution's epilogue on the fp32 accumulators:
//   out = bf16( relu?( acc * sc[co] + sh[co] (+ float(res[p][co])) ) )
// one rounding and one store per activation; no raw conv output, no statistics, no
// bn_apply launch.  sc / sh are the folded vectors of bn_affine.h (bn_fold below).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels/launchers.h"

namespace ddp_amd {

struct InferEpi {
  const float* sc = nullptr;    // [Cout] invstd * gamma
  const float* sh = nullptr;    // [Cout] beta - mean * sc
  const bf16_t* res = nullptr;  // optional NHWC residual of the output's shape
  int relu = 0;
};

// every forward plan of conv_gemm_plan (gathered GEMM, stem, staged 224 stem, halo, split K);
// `part` = fp32 workspace [splits][P][Cout] when pl.splits > 1
void conv_gemm_infer(const ConvGeom& g, const ConvPlan& pl, const bf16_t* X, const bf16_t* Wt,
                     const InferEpi& ie, bf16_t* Y, float* part, hipStream_t s);
void conv_halo_infer(const ConvGeom& g, int bp, int bc, int splits, const bf16_t* X, const bf16_t* Wt,
                     const InferEpi& ie, bf16_t* Y, float* part, hipStream_t s);

// sc = rsqrt(var + eps) * gamma, sh = fma(-mean, sc, beta) (bn_affine.h's definition)
void bn_fold(const float* running_mean, const float* running_var, const float* gamma, const float* beta,
             float eps, int C, float* sc, float* sh, hipStream_t s);

// One wave per row of fp32 logits [B][C] (any C >= 1): pred = lowest index among the maxima
// (0 when the maximum is NaN), loss = logsumexp(row) - row[label] (max-subtracted), correct =
// pred == label, correct5 = fewer than 5 classes rank before the label (row[j] > row[label],
// or equal with j < label).
void resnet_eval_tail(const float* logits, int C, int B, const long long* labels, int* pred, float* loss,
                      int* correct, int* correct5, hipStream_t s);
// tot[0] += sum correct, tot[1] += sum correct5; tot_loss[0] continues its fp64 running sum
// over loss[0, n) in index order (one block)
void resnet_eval_totals(const int* correct, const int* correct5, const float* loss, int n, long long* tot,
                        double* tot_loss, hipStream_t s);

}  // namespace ddp_amd
