// Epilogues of the 2 x 2-wave MFMA conv tiling, each written once: the gathered GEMM and the
// staged 224 stem (conv_gemm.hip), the 3x3 halo kernels (conv_halo.hip) and the pointwise
// GEMM (conv_pw.hip) all run 256 threads as 2 (channel) x 2 (pixel) waves, and accumulator
// (i, j) of a lane holds channels co + 16 i .. + 3 of the block's pixel column px + 16 j
// (co = block base + wco * (BC / 2) + 4 * (lane >> 4), px = wpx * (BP / 2) + (lane & 15)).
//
// What a kernel supplies is its pixel map: a callable j -> TilePx, the NHWC pixel index of
// column px + 16 j and whether that pixel exists.  Everything else - which LDS the statistics
// pass through, which slab row they land in, whether there is a bias - is an argument.
//
// The rule the BatchNorm and deferred-chain tests depend on lives here: a value is rounded to
// bf16 once (bias add, ReLU, rounding), and the statistics are sums of the STORED bf16 values
// with masked pixels counted as 0, in a fixed order: j ascending within a lane (squares by
// fmaf), sum16 over the 16 pixel lanes, pixel wave 0 + pixel wave 1.
#pragma once
#include "kernels/common.h"
#include "kernels/conv_infer.h"

namespace ddp_amd {

// K-slot permutation of the transposed (ds_read_b64_tr_b16) fragment read: fragment
// element j of lane group g holds k = 4g + j (j < 4) or 16 + 4g + (j - 4).  The matching
// non-transposed operand is stored to LDS in that order, so it stays one b128 read.
__device__ __forceinline__ int trk_pos(int k4) {  // LDS position of the 4-group starting at k = 4*k4
  return k4 < 4 ? 8 * k4 : 8 * (k4 - 4) + 4;
}

struct TilePx {
  bool live;  // the pixel exists (inside the tensor and the block's live columns)
  long idx;   // its NHWC pixel index
};

// Inference coefficients: the lane's 4 consecutive channels of each tile row.  Callers size
// the arrays INF ? TCO : 1 (training builds hold no registers for them) and request them
// before the K loop, so that they land during it.
template <int TCO>
__device__ __forceinline__ void infer_coef(const InferEpi& ie, int co, float4 (&sc)[TCO], float4 (&sh)[TCO]) {
#pragma unroll
  for (int i = 0; i < TCO; ++i) {
    sc[i] = *reinterpret_cast<const float4*>(ie.sc + co + 16 * i);
    sh[i] = *reinterpret_cast<const float4*>(ie.sh + co + 16 * i);
  }
}

// Inference store: relu?(acc * sc + sh (+ res)) rounded to bf16 once; the residual is one
// 8-byte load beside the 8-byte store.
template <int TCO, int TPX, typename PixFn>
__device__ __forceinline__ void infer_store(const f32x4 (&acc)[TCO][TPX], PixFn pix, const float4* isc,
                                            const float4* ish, const bf16_t* __restrict__ res, bool relu,
                                            bf16_t* __restrict__ Y, int C, int co) {
#pragma unroll
  for (int j = 0; j < TPX; ++j) {
    const TilePx p = pix(j);
    if (!p.live) continue;
#pragma unroll
    for (int i = 0; i < TCO; ++i) {
      const long off = p.idx * C + co + 16 * i;
      const float sc[4] = {isc[i].x, isc[i].y, isc[i].z, isc[i].w};
      const float sh[4] = {ish[i].x, ish[i].y, ish[i].z, ish[i].w};
      float v[4], rv[4] = {0.f, 0.f, 0.f, 0.f};
      if (res) unpack4(*reinterpret_cast<const uint2*>(res + off), rv);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = fmaf(acc[i][j][r], sc[r], sh[r]);
        if (res) v[r] += rv[r];
        if (relu) v[r] = fmaxf(v[r], 0.f);
      }
      *reinterpret_cast<uint2*>(Y + off) = pack4(v[0], v[1], v[2], v[3]);
    }
  }
}

// Split partial: fp32 into this split's [P][C] plane `dst`, 4 consecutive channels per lane = 16 B
template <int TCO, int TPX, typename PixFn>
__device__ __forceinline__ void part_store(const f32x4 (&acc)[TCO][TPX], PixFn pix, float* __restrict__ dst, int C,
                                           int co) {
#pragma unroll
  for (int j = 0; j < TPX; ++j) {
    const TilePx p = pix(j);
    if (!p.live) continue;
#pragma unroll
    for (int i = 0; i < TCO; ++i)
      *reinterpret_cast<float4*>(dst + p.idx * C + co + 16 * i) =
          make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
  }
}

// Training store: bf16 NHWC, and with STATS the lane's per-channel sum / sum of squares of
// the stored values.  BIAS: the kernel has a bias argument; it may still be null, and 0.f is
// added then, as those kernels always did (-0 becomes +0).
template <bool BIAS, bool RELU, bool STATS, int TCO, int TPX, typename PixFn>
__device__ __forceinline__ void train_store(const f32x4 (&acc)[TCO][TPX], PixFn pix, const float* __restrict__ bias,
                                            bf16_t* __restrict__ Y, int C, int co, float (&csum)[TCO][4],
                                            float (&csq)[TCO][4]) {
#pragma unroll
  for (int i = 0; i < TCO; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) csum[i][r] = csq[i][r] = 0.f;
#pragma unroll
  for (int j = 0; j < TPX; ++j) {
    const TilePx p = pix(j);
#pragma unroll
    for (int i = 0; i < TCO; ++i) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = acc[i][j][r];
        if (BIAS) v[r] += bias ? bias[co + 16 * i + r] : 0.f;
        if (RELU) v[r] = fmaxf(v[r], 0.f);
      }
      const uint2 pk = pack4(v[0], v[1], v[2], v[3]);
      if (p.live) *reinterpret_cast<uint2*>(Y + p.idx * C + co + 16 * i) = pk;
      if (STATS) {
        float q[4];
        unpack4(pk, q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = p.live ? q[r] : 0.f;
          csum[i][r] += x;
          csq[i][r] = fmaf(x, x, csq[i][r]);
        }
      }
    }
  }
}

// Statistics finish: the 16 pixel lanes by sum16, the two pixel waves through `s_st`, then the
// block's BC channels of one slab row [2][C] (`row` = that row + the block's first channel).
// cl = the lane's block-local channel of tile row 0.  No barrier follows the slab stores: a
// caller that writes s_st again synchronises first.
template <int BC, int TCO>
__device__ __forceinline__ void stats_finish(const float (&csum)[TCO][4], const float (&csq)[TCO][4],
                                             float (*s_st)[2][BC], int cl, int wpx, float* __restrict__ row, int C) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < TCO; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = sum16(csum[i][r]), b = sum16(csq[i][r]);
      if ((tid & 15) == 0) {
        s_st[wpx][0][cl + 16 * i + r] = a;
        s_st[wpx][1][cl + 16 * i + r] = b;
      }
    }
  __syncthreads();
  for (int c = tid; c < BC; c += 256) {
    st_wt(row + c, s_st[0][0][c] + s_st[1][0][c]);
    st_wt(row + C + c, s_st[0][1][c] + s_st[1][1][c]);
  }
}

// Data-gradient store: the split partial (`dst`: this split's plane), or bf16 with the
// optional ReLU mask by the layer input's activation (Xact > 0).
template <bool MASK_X, bool PART, int TCI, int TPX, typename PixFn>
__device__ __forceinline__ void dgrad_store(const f32x4 (&acc)[TCI][TPX], PixFn pix, const bf16_t* __restrict__ Xact,
                                            bf16_t* __restrict__ dX, float* __restrict__ dst, int C, int ci) {
  if constexpr (PART) {
    part_store(acc, pix, dst, C, ci);
  } else {
#pragma unroll
    for (int j = 0; j < TPX; ++j) {
      const TilePx p = pix(j);
      if (!p.live) continue;
#pragma unroll
      for (int i = 0; i < TCI; ++i) {
        const long off = p.idx * C + ci + 16 * i;
        float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        if (MASK_X) {
          float xm[4];
          unpack4(*reinterpret_cast<const uint2*>(Xact + off), xm);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = xm[r] > 0.f ? v[r] : 0.f;
        }
        *reinterpret_cast<uint2*>(dX + off) = pack4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

}  // namespace ddp_amd
