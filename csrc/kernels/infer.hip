// SimpleCNN inference: logits, prediction and per-image loss of a batch in ONE launch.
//
// The forward part is the training forward's body (conv3x3_fwd_body.inc.h) with conv1
// recomputed from the uint8 images (C1Src, optional index list), the MFMA conv2, bias + ReLU
// and the fc partial epilogue - and NOA2: the a2 store is compiled out (100 KB per image that
// nothing reads in inference).  No DZ, no MRG.  Each block publishes its partial logits
// [block][2][10] write-through.
//
// The tail never waits, so the grid needs no residency and any batch with B * 784 < 2^31
// runs: wave 0 (the only wave that stored partials) drains its stores and takes a ticket on
// the counter of each image the block touches (at most two; counters FWD_DZ_CNT_STRIDE ints
// apart; expected = the blocks touching the image, the level-3 wait's kb1 - kb0 + 1).  The
// block whose add returns the last ticket re-arms the counter and, on that wave, sums the
// image's partials with agent-scope loads in xent_logit_acc's fixed order, adds the fc bias,
// and evaluates the loss with xent_row_dl (unscaled) - the training step's arithmetic, so a
// row's loss has the bits the level-3 forward writes for the same image.  Prediction = the
// lowest-index maximum (a strict > scan from class 0).
//
// Hand-off (bn_tail.h; MI355X_MICROARCH.md hand-off table, first row): 4-byte write-through
// payload stored by one wave, that wave's vmcnt(0) drain, one relaxed agent-scope add per
// counter, the finisher told by the value its add returned, agent-scope (sc1) loads of every
// handed-off byte by the wave that added, no agent-scope fence.  The launcher asks for more
// than half a CU's LDS, so one block is resident per CU - the placement that row was
// measured at.
#include <stdexcept>

#include "kernels/conv3x3_fwd.h"
#include "kernels/xent_body.h"

namespace ddp_amd {

template <typename T, int NW>
__global__ __launch_bounds__(NW * 64, NW / 4) void simplecnn_infer_kernel(
    const T* __restrict__ Wt, const float* __restrict__ bias, const T* __restrict__ wfc,
    const float* __restrict__ fc_bias, int B, float* __restrict__ fc_part, int* __restrict__ img_cnt, C1Src c1,
    InferOut out) {
  constexpr int PXT = 1, NOF = 10, OCC = 1, GH = 28, GW = 28, GCI = 32, GCO = 64;
  constexpr bool RELU = true, A1X = true, DZ = false, MRG = false, NOA2 = true;
  const T* X = nullptr;
  T* Y = nullptr;
  int H = GH, W = GW, Cin = GCI, Cout = GCO;
  const FwdDz dzo{};
  const FwdMerge mg{};
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bx = (int)blockIdx.x, by = 0;
#include "kernels/conv3x3_fwd_body.inc.h"
  // ---- tail: tickets, and the finisher's logits / loss / prediction (wave 0 only: its
  // threads < 2 * NOF stored the block's partials above, no other wave stored anything)
  if (wave != 0) return;
  const int img0 = (int)(P0 / HW);
  const long plast = (P0 + CH < Ptot ? P0 + CH : Ptot) - 1;
  const int nimg = (int)(plast / HW) - img0 + 1;  // 1 or 2 (CH <= HW)
  float* s_lg = s_fc + NW * PXT * 4 * NOF;        // [2][NOF] logits (behind the tile sums)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial-logit stores are out
  bool last = false;
  if (lane < nimg) {
    const int im = img0 + lane;
    const int kb0 = im * HW / CH, kb1 = (im * HW + HW - 1) / CH;
    int* cnt = img_cnt + (long)im * FWD_DZ_CNT_STRIDE;
    const int prev = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == kb1 - kb0;  // expected - 1: every other block of the image has arrived
    if (last) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed
  }
  const unsigned long long fin = __ballot(last);  // bit s: this block finishes image img0 + s
  if (!fin) return;
  const int slot = lane >= NOF ? 1 : 0, o = lane - slot * NOF;
  const bool mine = lane < 2 * NOF && ((fin >> slot) & 1);
  const int im = img0 + slot;
  if (mine) {
    const float a = xent_logit_acc(im, o, HW, CH, NOF, [&](int i) {
      return __hip_atomic_load(fc_part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
    const float lg = fc_bias[o] + a;
    s_lg[lane] = lg;
    if (out.logits) out.logits[(long)im * NOF + o] = lg;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the row's logits (other lanes) are in LDS
  if (mine && o == 0) {
    const float* x = s_lg + slot * NOF;
    const int label = c1.labels[c1.bi.row(im, c1.bi.base())];
    float lossv = 0.f;
    (void)xent_row_dl(x, NOF, 0, label, 1.f, &lossv);
    int best = 0;
    float mx = x[0];
    for (int k = 1; k < NOF; ++k)
      if (x[k] > mx) { mx = x[k]; best = k; }
    out.pred[im] = best;
    out.correct[im] = best == label ? 1 : 0;
    out.loss_rows[im] = lossv;
  }
}

int infer_blocks(int B, int pxt) { return (int)(((long)B * 28 * 28 + 64 * pxt - 1) / (64 * pxt)); }

// more than half of the CU's 160 KiB: one resident block per CU (see the header)
static size_t infer_lds(int pxt, int es) {
  return std::max(conv3x3_fwd_lds(28, 32, pxt, true, es), (size_t)(80 * 1024 + 16));
}

template <typename T>
static void infer_launch(const T* Wt, const float* bias, const T* wfc, const float* fc_bias, int B, int pxt,
                         const C1Src& c1, float* fc_part, int* img_cnt, const InferOut& out, hipStream_t s) {
  const char* bad = !Wt || !bias ? "the conv2 weight / bias" : !wfc || !fc_bias ? "the fc weight (FCFRAG order) / bias"
                    : !c1.x || !c1.labels || !c1.w || !c1.b ? "the images / labels / conv1 parameters"
                    : !fc_part || !img_cnt ? "its scratch" : !out.pred || !out.correct || !out.loss_rows ? "its outputs"
                    : nullptr;
  if (bad) throw std::runtime_error(std::string("simplecnn_infer: missing ") + bad);
  if (pxt != 1 && pxt != 2) throw std::runtime_error("simplecnn_infer: pxt must be 1 or 2");
  if (B <= 0 || (long)B * 28 * 28 >= (1L << 31)) throw std::runtime_error("simplecnn_infer: need 0 < B * 784 < 2^31");
  const size_t lds = infer_lds(pxt, (int)sizeof(T));
  const dim3 grid((unsigned)infer_blocks(B, pxt));
  if (pxt == 2) {
    auto k = simplecnn_infer_kernel<T, 8>;
    lds_optin(k, lds);
    hipLaunchKernelGGL(k, grid, dim3(512), lds, s, Wt, bias, wfc, fc_bias, B, fc_part, img_cnt, c1, out);
  } else {
    auto k = simplecnn_infer_kernel<T, 4>;
    lds_optin(k, lds);
    hipLaunchKernelGGL(k, grid, dim3(256), lds, s, Wt, bias, wfc, fc_bias, B, fc_part, img_cnt, c1, out);
  }
}

void simplecnn_infer(const bf16_t* Wt, const float* bias, const bf16_t* wfc, const float* fc_bias, int B, int pxt,
                     const C1Src& c1, float* fc_part, int* img_cnt, const InferOut& out, hipStream_t s) {
  infer_launch<bf16_t>(Wt, bias, wfc, fc_bias, B, pxt, c1, fc_part, img_cnt, out, s);
}
void simplecnn_infer(const float* Wt, const float* bias, const float* wfc, const float* fc_bias, int B, int pxt,
                     const C1Src& c1, float* fc_part, int* img_cnt, const InferOut& out, hipStream_t s) {
  infer_launch<float>(Wt, bias, wfc, fc_bias, B, pxt, c1, fc_part, img_cnt, out, s);
}

// ---------------------------------------------------------------- totals of a batch
// One block: tot_correct[0] += sum correct[i]; tot_loss[0] = (((tot_loss[0] + loss[0]) +
// loss[1]) + ...) in fp64 - the running sum continues in INDEX order through every batch of a
// split, so the total does not depend on the batching and is reproducible; the host reads
// the pair once per split.
constexpr int TOT_THREADS = 256, TOT_CHUNK = 1024;
__global__ __launch_bounds__(TOT_THREADS) void infer_totals_kernel(const int* __restrict__ correct,
                                                                   const float* __restrict__ loss_rows, int n,
                                                                   long long* __restrict__ tot_correct,
                                                                   double* __restrict__ tot_loss) {
  __shared__ float s_loss[TOT_CHUNK];
  __shared__ int s_ok[TOT_CHUNK];
  long long c = 0;
  double l = 0.0;
  if (threadIdx.x == 0) { c = tot_correct[0]; l = tot_loss[0]; }
  for (int i0 = 0; i0 < n; i0 += TOT_CHUNK) {
    const int m = n - i0 < TOT_CHUNK ? n - i0 : TOT_CHUNK;
    for (int i = threadIdx.x; i < m; i += TOT_THREADS) {
      s_loss[i] = loss_rows[i0 + i];
      s_ok[i] = correct[i0 + i];
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) {
        l += (double)s_loss[i];
        c += s_ok[i];
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) { tot_correct[0] = c; tot_loss[0] = l; }
}

void infer_totals(const int* correct, const float* loss_rows, int n, long long* tot_correct, double* tot_loss,
                  hipStream_t s) {
  if (!correct || !loss_rows || !tot_correct || !tot_loss) throw std::runtime_error("infer_totals: null buffer");
  if (n <= 0) return;
  hipLaunchKernelGGL(infer_totals_kernel, dim3(1), dim3(TOT_THREADS), 0, s, correct, loss_rows, n, tot_correct,
                     tot_loss);
}

DDP_STAMPS_SETTER(stamps_set_infer)

}  // namespace ddp_amd
