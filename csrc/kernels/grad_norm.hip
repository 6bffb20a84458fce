// Global gradient norm for clip_grad_norm_-style clipping fused into the flat SGD step.
//
// grad_sqnorm_kernel reads the flat fp32 gradient once and leaves, in device memory, the
// L2 norm and the clip coefficient min(1, max_norm / (norm + 1e-6)) that the CLIP build of
// sgd_kernel (optim.hip) multiplies every gradient element by.  One launch, no float
// atomics, no agent-scope fences; bitwise reproducible and independent of the machine: the
// grid is a function of n alone.
//
// Exact order of the float operations (ddp_amd/ops/kernel_bounds.py replay_sqnorm replays
// it in numpy; the tests compare bit for bit):
//
//   n4 = n / 4 quads (16 bytes), G = grad_norm_blocks(n) = clamp(ceil(n4 / 1024), 1, 1024)
//   blocks of 256 threads, T = 256 G threads, global thread id t = 256 block + thread.
//   1. Thread t owns GN_QUADS = 4 x 4 = 16 accumulators acc[u][c], all +0.0f.  Pass
//      i = 0, 1, ... covers quads [4 T i, 4 T (i + 1)): quad q = 4 T i + u T + t, element
//      c of it, does acc[u][c] = fmaf(x, x, acc[u][c]) (one rounding); quads >= n4 are
//      skipped.  So each accumulator is a sequential chain over the passes.
//   2. Thread fold: s_u = (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]), then
//      th = (s_0 + s_1) + (s_2 + s_3).
//   3. Tail: thread j < n % 4 of block 0 does th = fmaf(x, x, th) with x = g[4 n4 + j].
//   4. Wave: wave_sum (common.h), a balanced pairwise tree over lanes 0..63: neighbours
//      (0+1), (2+3), ..., then pairs of those, ... (6 levels).
//   5. Block: ((w0 + w1) + w2) + w3 over its four waves -> partials[block] (write-through).
//   6. The block that arrives last: thread j sums ((P[j] + P[j+256]) + P[j+512]) + P[j+768]
//      (entries >= G count as +0.0f), then steps 4 and 5 again give the sum of squares S.
//   7. total_norm = sqrtf(S) and coef = min(1, max_norm / (total_norm + 1e-6f)), every
//      operation correctly rounded fp32 (torch.nn.utils.clip_grad_norm_'s arithmetic; a NaN
//      norm gives a NaN coefficient as torch's clamp does); steps += 1; clipped += coef < 1.
//
// Longest chain of roundings into S: passes + 2 (fold) + 2 + 1 (tail) + 6 + 3 + 3 + 6 + 3
// = passes + 26 (kernel_bounds.sqnorm_bound).
//
// In flight: 4 independent 16-byte loads per thread and pass; at the full grid (4 blocks =
// 16 waves per CU on 256 CUs) that is 64 KiB per CU, the depth at which a streaming read
// hides an HBM miss (MI355X: ~72 KiB per CU reads within a few percent of the L2-share curve).
#include "kernels/bn_tail.h"
#include "kernels/common.h"
#include "kernels/launchers.h"

namespace ddp_amd {

int grad_norm_blocks(long n) {
  const long per = (long)GN_THREADS * GN_QUADS;
  const long b = ((n >> 2) + per - 1) / per;
  return (int)(b < 1 ? 1 : (b > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : b));
}

// fixed-order sum over the block's 256 threads (steps 4 and 5); the result is valid in thread 0
__device__ __forceinline__ float gn_block_sum(float v, float* s_w) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(GN_THREADS) void grad_sqnorm_kernel(const float* __restrict__ g, long n,
                                                                 float max_norm,
                                                                 float* __restrict__ partials,
                                                                 int* __restrict__ ticket,
                                                                 ClipStats* __restrict__ out) {
  static_assert(GN_THREADS == 256 && GN_QUADS == 4 && GN_MAX_BLOCKS <= 4 * GN_THREADS,
                "the folds below are written for 4 waves, 4 quads and <= 1024 partials");
  __shared__ float s_w[4];
  __shared__ int s_last;
  const int G = gridDim.x;
  const long n4 = n >> 2;
  const long T = (long)G * GN_THREADS;
  const long t = (long)blockIdx.x * GN_THREADS + threadIdx.x;
  float4 acc[GN_QUADS];
#pragma unroll
  for (int u = 0; u < GN_QUADS; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long base = 0; base < n4; base += GN_QUADS * T) {
    float4 v[GN_QUADS];
#pragma unroll
    for (int u = 0; u < GN_QUADS; ++u) {  // all loads of the pass issued before the first use
      // branch-free: a quad past the end loads quad n4 - 1 (n4 >= 1 inside the loop) and is
      // zeroed below - a guarded load compiles to a branch with its own vmcnt(0) wait, one
      // load in flight at a time
      const long q = base + u * T + t;
      v[u] = reinterpret_cast<const float4*>(g)[q < n4 ? q : n4 - 1];
    }
#pragma unroll
    for (int u = 0; u < GN_QUADS; ++u) {
      if (base + u * T + t >= n4) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      acc[u].x = fmaf(v[u].x, v[u].x, acc[u].x);
      acc[u].y = fmaf(v[u].y, v[u].y, acc[u].y);
      acc[u].z = fmaf(v[u].z, v[u].z, acc[u].z);
      acc[u].w = fmaf(v[u].w, v[u].w, acc[u].w);
    }
  }
  float s[GN_QUADS];
#pragma unroll
  for (int u = 0; u < GN_QUADS; ++u) s[u] = (acc[u].x + acc[u].y) + (acc[u].z + acc[u].w);
  float th = (s[0] + s[1]) + (s[2] + s[3]);
  // scalar tail (as sgd_kernel: the first threads of block 0)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float x = g[(n4 << 2) + threadIdx.x];
    th = fmaf(x, x, th);
  }
  const float bsum = gn_block_sum(th, s_w);
  if (threadIdx.x == 0) st_wt(partials + blockIdx.x, bsum);
  if (!last_arrival(ticket, G, &s_last)) return;  // (its barriers also fence s_w for reuse)

  float p[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = threadIdx.x + k * GN_THREADS;
    p[k] = j < G ? ld_agent(partials + j) : 0.f;
  }
  const float S = gn_block_sum(((p[0] + p[1]) + p[2]) + p[3], s_w);
  if (threadIdx.x == 0) {
    // correctly rounded fp32 square root whatever the compiler's fp32 sqrt expansion is (the
    // intrinsic compiled to the 1-ulp v_sqrt_f32): the root of a float, taken in double and
    // rounded to float, is the correctly rounded float root (53 >= 2 * 24 + 2 bits)
    const float norm = (float)sqrt((double)S);
    const float q = __fdiv_rn(max_norm, norm + 1e-6f);
    const float coef = q > 1.f ? 1.f : q;  // NaN stays NaN (torch.clamp(max=1))
    out->total_norm = norm;
    out->coef = coef;
    out->steps += 1;
    out->clipped += coef < 1.f ? 1 : 0;
  }
}

void grad_sqnorm(const float* g, long n, float max_norm, float* partials, int* ticket, ClipStats* out,
                 hipStream_t s) {
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)grad_norm_blocks(n)), dim3(GN_THREADS), 0, s, g, n,
                     max_norm, partials, ticket, out);
}

}  // namespace ddp_amd
