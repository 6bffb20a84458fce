// Pointwise convolution (1x1, stride 1, pad 0; NHWC bf16) as the plain GEMM it is - the
// bottleneck blocks' conv1 / conv3 and layer 1's stride-1 downsample (about half of
// ResNet-50's FLOPs).  With P = N*H*W pixels the input is a row-major [P][Cin] matrix, the
// OHWI weight is [Cout][Cin] and the output is [P][Cout]: the im2col of such a layer is the
// identity, so there is no ConvGeom index math anywhere in these kernels (the gathered
// conv_gemm_fwd_kernel recomputes n / oh / ow / ih / iw and a bounds predicate per K-step).
// Scope: Cin % 64 == 0, Cout % 64 == 0, both <= 2048 (conv_pw_plan's `ok`).
//
// Forward   Y[p][co] = sum_ci act(X)[p][ci] * W[co][ci]
//   Output channels on the MFMA rows, pixels on the columns (common.h), 4 waves as 2 (co) x
//   2 (px) over a BP-pixel x BC-channel block tile.  K-step = 64 input channels = two
//   v_mfma_f32_16x16x32_bf16 per accumulator per barrier (the gathered kernel: 32 channels,
//   one).  Both operand tiles are rows of 128 contiguous bytes: a thread loads 16 bytes, 8
//   consecutive threads one row; the only predicate is the pixel tail p < P.  The tiles are
//   double-buffered through LDS at a row stride of 80 elements (40 dwords == 8 mod 16: the
//   b128 fragment reads are conflict-free), and the next K-step's global loads are issued
//   before this step's MFMAs.  No split-K: K <= 2048 is at most 32 K-steps.
//   AFF: X is a producer's raw conv output with a deferred BatchNorm + ReLU (BnAffine).  The
//   block forms sc / sh of all Cin channels once into LDS (bn_affine8) and applies bn_relu8
//   in registers between the global load and the LDS store - bn_affine.h's one definition,
//   so the staged operand is bitwise what bn_apply would have stored and the result is
//   bitwise the non-AFF kernel's on the materialised activation.
//   EPI: PW_PLAIN bf16 store; PW_STATS bf16 store + per-block per-channel sum / sum of
//   squares of the STORED values into the slab [grid_x][2][Cout] (conv_gemm_fwd_kernel's
//   layout and st_wt stores: bn_finalize reads it unchanged); PW_INFER conv_infer.h's
//   InferEpi, relu?(acc * sc + sh (+ res)) rounded once.
//
// Weight gradient   dW[co][ci] = sum_p dY[p][co] * act(X)[p][ci]     (K = pixels)
//   Block tile BM co x BN ci, 4 waves of (BM/2) x (BN/2); a K-step stages 64 pixels of dY
//   [64][BM] and X [64][BN] exactly as stored (pixel rows, 16-byte pieces; row stride BM+16 /
//   BN+16 = an odd multiple of 8 dwords) and both MFMA fragments are read with
//   ds_read_b64_tr_b16.  Both operands take the transposed read, so both see the same K-slot
//   order (conv_epilogue.h trk_pos: k = 4g + j, 16 + 4g + j) and no operand is permuted when
//   stored.  AFF applies the deferred affine to X while staging (a thread keeps one channel
//   group for the whole K loop: its sc / sh stay in 16 registers).  Pixels are split into
//   chunks of `ppc` on grid.z: one chunk writes dW (fp32, `accum` adds to it), several write
//   a slab [chunks][Cout*Cin] that grad_reduce sums in fixed order - no atomics, bitwise run
//   to run.
//
// The data gradient stays on conv_gemm_dgrad_kernel (it reads dY and W only, neither is ever
// deferred); a pointwise dgrad in this family is the follow-up.
#include <algorithm>
#include <stdexcept>

#include "kernels/bn_affine.h"
#include "kernels/common.h"
#include "kernels/conv_epilogue.h"
#include "kernels/conv_infer.h"
#include "kernels/launchers.h"

namespace ddp_amd {

constexpr int PW_KS = 64;          // K-step: input channels (forward), pixels (weight gradient)
constexpr int PW_RS = PW_KS + 16;  // forward LDS row stride (elements)
enum { PW_PLAIN = 0, PW_STATS = 1, PW_INFER = 2 };

template <int BP, int BC, bool AFF, int EPI>
__global__ __launch_bounds__(256) void conv_pw_fwd_kernel(const bf16_t* __restrict__ X,
                                                          const bf16_t* __restrict__ Wt,
                                                          bf16_t* __restrict__ Y, float* __restrict__ stats,
                                                          int P, int Cin, int Cout, BnAffine aff, InferEpi ie) {
  __shared__ __attribute__((aligned(16))) bf16_t sA[2][BC * PW_RS];
  __shared__ __attribute__((aligned(16))) bf16_t sB[2][BP * PW_RS];
  extern __shared__ __attribute__((aligned(16))) float s_aff[];  // AFF: sc[Cin], sh[Cin]
  constexpr int TCO = BC / 32, TPX = BP / 32;  // 16 x 16 tiles per wave
  constexpr int NA = BC / 32, NB = BP / 32;    // 16-byte pieces per thread and K-step
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wco = wave >> 1, wpx = wave & 1;
  const int3 bk = xcd_block3();  // XCD-contiguous block order (pixel tiles of one channel tile share an L2)
  const int p0 = bk.x * BP, co0 = bk.y * BC;
  const int nk = Cin / PW_KS;
  const int srow = tid >> 3, sch = (tid & 7) * 8;  // staging: row (+ 32 per piece), channel offset

  auto load_k = [&](int ks, bf16x8* ra, bf16x8* rb) {
    const int k0 = ks * PW_KS + sch;
#pragma unroll
    for (int u = 0; u < NA; ++u) ra[u] = ld8(Wt + (long)(co0 + srow + 32 * u) * Cin + k0);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int p = p0 + srow + 32 * u;
      rb[u] = p < P ? ld8(X + (long)p * Cin + k0) : zero8();
    }
  };
  auto store_k = [&](int buf, int ks, const bf16x8* ra, const bf16x8* rb) {
#pragma unroll
    for (int u = 0; u < NA; ++u) *reinterpret_cast<bf16x8*>(&sA[buf][(srow + 32 * u) * PW_RS + sch]) = ra[u];
    float sc[8], sh[8];
    if constexpr (AFF) {
      const float* a = s_aff + ks * PW_KS + sch;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 c4 = *reinterpret_cast<const float4*>(a + 4 * h);
        const float4 h4 = *reinterpret_cast<const float4*>(a + Cin + 4 * h);
        sc[4 * h] = c4.x; sc[4 * h + 1] = c4.y; sc[4 * h + 2] = c4.z; sc[4 * h + 3] = c4.w;
        sh[4 * h] = h4.x; sh[4 * h + 1] = h4.y; sh[4 * h + 2] = h4.z; sh[4 * h + 3] = h4.w;
      }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      bf16x8 v = rb[u];
      if constexpr (AFF) {
        if (p0 + srow + 32 * u < P) v = bn_relu8(v, sc, sh);  // the tail rows stay zero
      }
      *reinterpret_cast<bf16x8*>(&sB[buf][(srow + 32 * u) * PW_RS + sch]) = v;
    }
  };

  f32x4 acc[TCO][TPX];
#pragma unroll
  for (int i = 0; i < TCO; ++i)
#pragma unroll
    for (int j = 0; j < TPX; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  bf16x8 ra[NA], rb[NB];
  load_k(0, ra, rb);
  if constexpr (AFF) {  // sc / sh of every input channel, while the first tiles are in flight
    for (int c0 = tid * 8; c0 < Cin; c0 += 256 * 8) {
      float sc[8], sh[8];
      bn_affine8(aff.invstd, aff.gamma, aff.mean, aff.beta, c0, sc, sh);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s_aff[c0 + j] = sc[j];
        s_aff[Cin + c0 + j] = sh[j];
      }
    }
    __syncthreads();
  }
  // PW_INFER: the lane's 4 consecutive output channels of each tile row, requested here so
  // that they land during the K loop
  const int cl = wco * (BC / 2) + 4 * (lane >> 4);  // the lane's block-local channel of tile row 0
  float4 isc[EPI == PW_INFER ? TCO : 1], ish[EPI == PW_INFER ? TCO : 1];
  if constexpr (EPI == PW_INFER) infer_coef(ie, co0 + cl, isc, ish);
  store_k(0, 0, ra, rb);
  __syncthreads();
  const int kofs = 8 * (lane >> 4), col = lane & 15;
  for (int ks = 0; ks < nk; ++ks) {
    const int cur = ks & 1;
    const bool more = ks + 1 < nk;  // block-uniform
    if (more) load_k(ks + 1, ra, rb);
#pragma unroll
    for (int kk = 0; kk < PW_KS / 32; ++kk) {
      bf16x8 a[TCO], b[TPX];
#pragma unroll
      for (int i = 0; i < TCO; ++i)
        a[i] = *reinterpret_cast<const bf16x8*>(&sA[cur][(wco * (BC / 2) + 16 * i + col) * PW_RS + 32 * kk + kofs]);
#pragma unroll
      for (int j = 0; j < TPX; ++j)
        b[j] = *reinterpret_cast<const bf16x8*>(&sB[cur][(wpx * (BP / 2) + 16 * j + col) * PW_RS + 32 * kk + kofs]);
#pragma unroll
      for (int i = 0; i < TCO; ++i)
#pragma unroll
        for (int j = 0; j < TPX; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
    }
    if (more) store_k(cur ^ 1, ks + 1, ra, rb);  // buffer cur ^ 1 was last read a step ago
    __syncthreads();
  }

  // ---- epilogue (conv_epilogue.h); the block's pixel columns are consecutive rows of Y
  const int px = p0 + wpx * (BP / 2) + col;
  auto pix = [&](int j) { return TilePx{px + 16 * j < P, px + 16 * j}; };
  if constexpr (EPI == PW_INFER) {
    infer_store(acc, pix, isc, ish, ie.res, ie.relu != 0, Y, Cout, co0 + cl);
  } else {
    float csum[TCO][4], csq[TCO][4];
    train_store<false, false, EPI == PW_STATS>(acc, pix, nullptr, Y, Cout, co0 + cl, csum, csq);
    if constexpr (EPI == PW_STATS) {
      __shared__ float s_st[2][2][BC];
      stats_finish(csum, csq, s_st, cl, wpx, stats + (long)bk.x * 2 * Cout + co0, Cout);
    }
  }
}

// ---------------------------------------------------------------- weight gradient
template <int BM, int BN, bool AFF>
__global__ __launch_bounds__(256) void conv_pw_wgrad_kernel(const bf16_t* __restrict__ dY,
                                                            const bf16_t* __restrict__ X,
                                                            float* __restrict__ out, int P, int Cin, int Cout,
                                                            int ppc, int accum, BnAffine aff) {
  constexpr int RD = BM + 16, RX = BN + 16;
  constexpr int DPT = BM * PW_KS / 2048, XPT = BN * PW_KS / 2048;  // 16-byte pieces per thread and K-step
  constexpr int DROWS = 2048 / BM, XROWS = 2048 / BN;              // pixel rows one round of 256 pieces covers
  constexpr int TA = BM / 32, TB = BN / 32;
  __shared__ __attribute__((aligned(16))) bf16_t sD[2][PW_KS * RD];
  __shared__ __attribute__((aligned(16))) bf16_t sX[2][PW_KS * RX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co0 = blockIdx.x * BM, ci0 = blockIdx.y * BN;
  const int pbeg = blockIdx.z * ppc, pend = min(P, pbeg + ppc);
  // a thread's channel group is the same in every round (256 % (BM/8) == 0): only the pixel moves
  const int dsp = tid / (BM / 8), dsc = (tid % (BM / 8)) * 8;
  const int xsp = tid / (BN / 8), xsc = (tid % (BN / 8)) * 8;
  float sc[8], sh[8];
  if constexpr (AFF) bn_affine8(aff.invstd, aff.gamma, aff.mean, aff.beta, ci0 + xsc, sc, sh);
  auto load = [&](int pk, bf16x8* vd, bf16x8* vx) {
#pragma unroll
    for (int u = 0; u < DPT; ++u) {
      const int p = pk + dsp + DROWS * u;
      vd[u] = p < pend ? ld8(dY + (long)p * Cout + co0 + dsc) : zero8();
    }
#pragma unroll
    for (int u = 0; u < XPT; ++u) {
      const int p = pk + xsp + XROWS * u;
      vx[u] = p < pend ? ld8(X + (long)p * Cin + ci0 + xsc) : zero8();
    }
  };
  auto store = [&](int buf, int pk, const bf16x8* vd, const bf16x8* vx) {
#pragma unroll
    for (int u = 0; u < DPT; ++u) *reinterpret_cast<bf16x8*>(&sD[buf][(dsp + DROWS * u) * RD + dsc]) = vd[u];
#pragma unroll
    for (int u = 0; u < XPT; ++u) {
      bf16x8 v = vx[u];
      if constexpr (AFF) {
        if (pk + xsp + XROWS * u < pend) v = bn_relu8(v, sc, sh);  // pixels past the chunk stay zero
      }
      *reinterpret_cast<bf16x8*>(&sX[buf][(xsp + XROWS * u) * RX + xsc]) = v;
    }
  };
  const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);
  const int gq = lane >> 4, i16 = lane & 15, q = i16 >> 2, pq = i16 & 3;
  f32x4 acc[TA][TB];
#pragma unroll
  for (int a = 0; a < TA; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bf16x8 vd[DPT], vx[XPT];
  load(pbeg, vd, vx);
  store(0, pbeg, vd, vx);
  __syncthreads();
  int cur = 0;
  const int kA = 4 * gq + q, kB = 16 + 4 * gq + q;  // the transposed read's K rows (trk_pos order)
  for (int pk = pbeg; pk < pend; pk += PW_KS) {
    const bool more = pk + PW_KS < pend;  // block-uniform
    if (more) load(pk + PW_KS, vd, vx);
#pragma unroll
    for (int kk = 0; kk < PW_KS / 32; ++kk) {
      bf16x8 fa[TA], fb[TB];
#pragma unroll
      for (int a = 0; a < TA; ++a) {
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)&sD[cur][(32 * kk + kA) * RD + wm + 16 * a + 4 * pq]);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)&sD[cur][(32 * kk + kB) * RD + wm + 16 * a + 4 * pq]);
        fa[a] = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int b = 0; b < TB; ++b) {
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)&sX[cur][(32 * kk + kA) * RX + wn + 16 * b + 4 * pq]);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)&sX[cur][(32 * kk + kB) * RX + wn + 16 * b + 4 * pq]);
        fb[b] = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b) acc[a][b] = mfma16(fa[a], fb[b], acc[a][b]);
    }
    if (more) store(cur ^ 1, pk + PW_KS, vd, vx);
    __syncthreads();
    cur ^= 1;
  }
  // accumulator (a, b, r) = dW[co0 + wm + 16 a + 4 gq + r][ci0 + wn + 16 b + i16]
  float* o = out + (long)blockIdx.z * Cout * Cin + (long)(co0 + wm + 4 * gq) * Cin + ci0 + wn + i16;
  float old[TA][TB][4];
  if (accum) {  // all prior values in flight at once, then the stores
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int b = 0; b < TB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) old[a][b][r] = o[(long)(16 * a + r) * Cin + 16 * b];
  }
#pragma unroll
  for (int a = 0; a < TA; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        o[(long)(16 * a + r) * Cin + 16 * b] = accum ? old[a][b][r] + acc[a][b][r] : acc[a][b][r];
}

// ---------------------------------------------------------------- host side
// Forward block tile, from scripts/resnet50_bench.py --tiles over ResNet-50 at batch 32
// (profiles/resnet50/README.md):
//  * Cin >= 512 (8+ K-steps): the widest offered tile whose grid still gives every one of the
//    256 CUs a block - a 128-wide tile loads half the operand bytes per output of a 64 x 64
//    one.  Layer 4 (P = 1568): 128 x 64 for Cout = 2048 (416 blocks, 14.8 against 16.4 us),
//    64 x 64 for Cout = 512 (200 blocks, the most this GEMM has without split-K; 20.4 against
//    28.9 us for the 52 blocks of 128 x 128).
//  * Cin <= 256 (at most 4 K-steps): 64 x 64.  These layers run at the memory rate - layer 1's
//    P = 100352 reads 13 MB and writes 51 MB for 3.3 GFLOP - and three resident 41 KB blocks
//    per CU keep more loads and stores in flight than two 80 KB ones: 64 -> 256 at P = 100352
//    takes 25.6 us against 36.3 us with 128 x 128 tiles; the operand reuse is in L2 either way.
// bp / bc != 0 force one of the offered tiles.
PwPlan conv_pw_plan(long P, int Cin, int Cout, int bp, int bc) {
  PwPlan pl{};
  static const int tiles[3][2] = {{128, 128}, {128, 64}, {64, 64}};
  if (P <= 0 || Cin % 64 || Cout % 64 || Cin < 64 || Cout < 64 || Cin > 2048 || Cout > 2048) return pl;
  for (const auto& t : tiles) {
    if (Cout % t[1]) continue;
    if ((bp || bc) && (bp != t[0] || bc != t[1])) continue;
    if (!(bp || bc) && Cin <= 256 && t[0] != 64) continue;
    pl.ok = 1;
    pl.bp = t[0];
    pl.bc = t[1];
    pl.grid_x = (int)((P + t[0] - 1) / t[0]);
    pl.grid_y = Cout / t[1];
    if (bp || bc || (long)pl.grid_x * pl.grid_y >= 256) break;
  }
  return pl;
}

static void pw_check(const PwPlan& pl, long P, int Cin, int Cout) {
  if (!pl.ok || Cout % pl.bc || (long)pl.grid_x * pl.bp < P || pl.grid_y * pl.bc != Cout || Cin % PW_KS)
    throw std::runtime_error("conv_pw: the plan does not cover this layer");
}

void conv_pw_fwd(const PwPlan& pl, const bf16_t* X, const bf16_t* Wt, bf16_t* Y, float* stats, long P,
                 int Cin, int Cout, const BnAffine* aff, hipStream_t s) {
  pw_check(pl, P, Cin, Cout);
  const dim3 grid(pl.grid_x, pl.grid_y);
  const bool af = aff && aff->mean;
  const size_t lds = af ? sizeof(float) * 2 * Cin : 0;
  const BnAffine a = af ? *aff : BnAffine{};
#define PWF(BP, BC, AF, EP) hipLaunchKernelGGL((conv_pw_fwd_kernel<BP, BC, AF, EP>), grid, dim3(256), lds, s, X, Wt, Y, stats, (int)P, Cin, Cout, a, InferEpi{})
#define PWF_T(BP, BC)                                                             \
  do {                                                                            \
    if (af) { if (stats) PWF(BP, BC, true, PW_STATS); else PWF(BP, BC, true, PW_PLAIN); } \
    else { if (stats) PWF(BP, BC, false, PW_STATS); else PWF(BP, BC, false, PW_PLAIN); }  \
  } while (0)
  if (pl.bp == 128) { if (pl.bc == 128) PWF_T(128, 128); else PWF_T(128, 64); }
  else PWF_T(64, 64);
#undef PWF_T
#undef PWF
}

void conv_pw_infer(const PwPlan& pl, const bf16_t* X, const bf16_t* Wt, const InferEpi& ie, bf16_t* Y, long P,
                   int Cin, int Cout, hipStream_t s) {
  pw_check(pl, P, Cin, Cout);
  if (!ie.sc || !ie.sh) throw std::runtime_error("conv_pw_infer: the folded BatchNorm vectors are required");
  const dim3 grid(pl.grid_x, pl.grid_y);
  float* nof = nullptr;
#define PWI(BP, BC) hipLaunchKernelGGL((conv_pw_fwd_kernel<BP, BC, false, PW_INFER>), grid, dim3(256), 0, s, X, Wt, Y, nof, (int)P, Cin, Cout, BnAffine{}, ie)
  if (pl.bp == 128) { if (pl.bc == 128) PWI(128, 128); else PWI(128, 64); }
  else PWI(64, 64);
#undef PWI
}

// Weight-gradient tile and pixels per chunk.  Tile: the widest of 128 x 128, 128 x 64 (co x
// ci) and 64 x 64 that gives >= 256 tiles, so the big layers (layer 4: 2048 x 512 = 256 tiles
// of 64 x 64) fill the GPU with ONE chunk and write the gradient itself.  When even 64 x 64
// gives fewer (layer 1: 64 x 256 = 4 tiles over 100352 pixels) the grid has to come from
// pixel chunks, and for a given number of blocks the slab is blocks x tile area x 4 bytes: the
// 64 x 64 tile is kept (a quarter of the 128 x 128 slab) and the pixels are chunked until the
// grid has ~512 blocks (two per CU), each chunk a multiple of the 64-pixel K-step and at
// least 256 pixels (4 K-steps) long.
// Slab cap: chunks * Cout * Cin * 4 B <= 16 MiB.  The slab is written once and read once by
// grad_reduce; 16 MiB each way is ~8 us at HBM rate, about what the largest chunked layers'
// own MFMA work takes, and it stays inside the 256 MiB of last-level cache with the step's
// activations.  Past it, fewer and longer chunks win.  (512 blocks of 64 x 64 are 8 MiB.)
// bm / bn / ppc != 0 force the tile / the chunk length.
PwWgradPlan conv_pw_wgrad_plan(long P, int Cin, int Cout, int bm, int bn, int ppc) {
  PwWgradPlan pl{};
  static const int tiles[3][2] = {{128, 128}, {128, 64}, {64, 64}};
  if (P <= 0 || Cin % 64 || Cout % 64 || Cin < 64 || Cout < 64 || Cin > 2048 || Cout > 2048) return pl;
  for (const auto& t : tiles) {
    if (Cout % t[0] || Cin % t[1]) continue;
    if ((bm || bn) && (bm != t[0] || bn != t[1])) continue;
    pl.bm = t[0];
    pl.bn = t[1];
    if (bm || bn || (long)(Cout / t[0]) * (Cin / t[1]) >= 256) break;  // else: falls to 64 x 64
  }
  if (!pl.bm) return pl;
  if (ppc <= 0) {
    const long tl = (long)(Cout / pl.bm) * (Cin / pl.bn);
    long chunks = tl >= 256 ? 1 : 512 / tl;
    chunks = std::min(chunks, std::max(1L, (16L << 20) / ((long)Cout * Cin * 4)));
    long v = (P + chunks - 1) / chunks;
    v = std::max(256L, (v + PW_KS - 1) / PW_KS * PW_KS);
    ppc = (int)std::min<long>(v, (P + PW_KS - 1) / PW_KS * PW_KS);
  }
  pl.ppc = ppc;
  pl.chunks = (int)((P + ppc - 1) / ppc);
  return pl;
}

void conv_pw_wgrad(const PwWgradPlan& pl, const bf16_t* dY, const bf16_t* X, float* out, long P, int Cin,
                   int Cout, bool accum, const BnAffine* aff, hipStream_t s) {
  if (!pl.bm || Cout % pl.bm || Cin % pl.bn || pl.ppc <= 0 || (long)pl.chunks * pl.ppc < P)
    throw std::runtime_error("conv_pw_wgrad: the plan does not cover this layer");
  const dim3 grid(Cout / pl.bm, Cin / pl.bn, pl.chunks);
  const int acc = (accum && pl.chunks == 1) ? 1 : 0;
  const bool af = aff && aff->mean;
  const BnAffine a = af ? *aff : BnAffine{};
#define PWW(M, N, AF) hipLaunchKernelGGL((conv_pw_wgrad_kernel<M, N, AF>), grid, dim3(256), 0, s, dY, X, out, (int)P, Cin, Cout, pl.ppc, acc, a)
#define PWW_T(M, N) do { if (af) PWW(M, N, true); else PWW(M, N, false); } while (0)
  if (pl.bm == 128) { if (pl.bn == 128) PWW_T(128, 128); else PWW_T(128, 64); }
  else PWW_T(64, 64);
#undef PWW_T
#undef PWW
}

}  // namespace ddp_amd
