// Native host runtime of ddp_amd: RCCL communicator, bucketed gradient reducer and
// the fused SimpleCNN training-step engine (with hipGraph capture).
// Plain HIP host API + RCCL; no torch types (the pybind layer adapts tensors).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "kernels/launchers.h"
#include "runtime/bucket_state.h"
#include "runtime/step_plan.h"

#define DDP_HIP_CHECK(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__) + ": " #expr);  \
  } while (0)

#define DDP_NCCL_CHECK(expr)                                                             \
  do {                                                                                   \
    ncclResult_t _r = (expr);                                                            \
    if (_r != ncclSuccess)                                                               \
      throw std::runtime_error(std::string("RCCL error ") + ncclGetErrorString(_r) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__) + ": " #expr);  \
  } while (0)

namespace ddp_amd {

// Set from Python's atexit: once the interpreter is shutting down, destructors leak
// their HIP/RCCL handles instead of calling into a runtime that may be torn down.
void mark_exiting();
bool process_exiting();

// ---------------------------------------------------------------- RCCL communicator
// One communicator per process group, bootstrapped from an ncclUniqueId that rank 0
// creates and the Python layer distributes through the c10d TCPStore.
class Comm {
 public:
  static std::string new_unique_id();
  Comm(const std::string& uid, int rank, int world, int device);
  ~Comm();
  Comm(const Comm&) = delete;
  Comm& operator=(const Comm&) = delete;

  int rank() const { return rank_; }
  int world() const { return world_; }
  // dtype: 0 = f32, 1 = bf16, 2 = i32, 3 = i64, 4 = u8; op: 0 = sum, 1 = avg, 2 = max
  void all_reduce(void* buf, size_t count, int dtype, int op, hipStream_t s);
  void broadcast(void* buf, size_t count, int dtype, int root, hipStream_t s);
  void all_gather(const void* send, void* recv, size_t count, int dtype, hipStream_t s);
  void reduce_scatter(const void* send, void* recv, size_t count, int dtype, int op, hipStream_t s);
  // fp32 SUM of every rank's buffer times `scale` (RCCL's pre-multiplied sum: the multiply
  // happens inside the reduction - DDP's prescale-by-1/world without a separate pass)
  void all_reduce_premul(float* buf, size_t count, float scale, hipStream_t s);

 private:
  ncclComm_t comm_ = nullptr;
  int rank_ = 0, world_ = 1;
  std::vector<std::pair<float, ncclRedOp_t>> premul_;  // one op per scale, destroyed with the comm
};

// ---------------------------------------------------------------- direct xGMI all-reduce
// One channel per gradient bucket (a fixed [off, off + n) range of the gradient buffer);
// see xgmi.cpp / kernels/allreduce.hip.  Producers of a bucket must write it with
// system-scope stores (peers read it over xGMI right after the kernel boundary).
// What one rank's kernel arguments of a channel are filled from: the bucket, and every rank's
// data / stage / signal pointers as this rank addresses them.
struct XgmiPlan {
  long off, n, slice;
  bool oneshot;
  float* const* data;
  float* const* stage;
  unsigned* const* sig;
};
// the one place that fills XgmiArgs (XgmiComm::make_args and XgmiLoopback::all_reduce)
XgmiArgs xgmi_fill_args(const XgmiPlan& c, int rank, int world, double timeout_s, const SgdArgs& sgd, float* params,
                        float* mbuf, const ShadowSet& sh, int* step_ctr, float scale, bool publish, float prescale);

class XgmiComm {
 public:
  XgmiComm(int rank, int world, int device);
  ~XgmiComm();
  XgmiComm(const XgmiComm&) = delete;
  XgmiComm& operator=(const XgmiComm&) = delete;
  // grid_cap: most blocks for this channel's kernel (0: XGMI_GRID_CAP); a channel whose
  // all-reduce overlaps compute keeps its spinning grid small
  int add_channel(long off, long n, bool oneshot = false, int grid_cap = 0);
  int blocks(int channel) const { return ch_.at(channel).blocks; }
  std::string bus_id() const;  // PCI bus id of the device (ranks sharing a GPU compare these)
  bool oneshot(int channel) const { return ch_.at(channel).oneshot; }
  void set_data(float* data, long numel);
  std::string export_handles() const;
  void import_handles(const std::vector<std::string>& all);
  // publish: the bucket's producers used plain stores (module path): each block re-stores
  // its part system-scope before the entry barrier (no effect on one-shot channels, which
  // always copy the bucket to their stage buffer that way)
  // prescale (publish / one-shot only): my values times prescale before the rank-order sum
  void all_reduce(int channel, hipStream_t s, float scale = 1.f, bool publish = false, float prescale = 1.f);
  // the same, with SGD fused into the all-gather (see XgmiArgs)
  void all_reduce_sgd(int channel, hipStream_t s, const SgdArgs& sgd, float* params, float* mbuf,
                      const ShadowSet& sh, int* step_ctr, float scale = 1.f, bool publish = false,
                      float prescale = 1.f);
  // the kernel arguments all_reduce_sgd would launch with (the in-launch all-reduce role of
  // the conv backward runs the same body from them, with blocks(channel) blocks)
  XgmiArgs make_args(int channel, const SgdArgs& sgd, float* params, float* mbuf, const ShadowSet& sh,
                     int* step_ctr, float scale = 1.f, bool publish = false, float prescale = 1.f) const;
  // Two channels' all-reduces in ONE launch - the engine's dist_mode 3 kernel
  // (xgmi_allreduce_pair) as a standalone call: blocks [0, blocks(ch0)) run ch0, the rest
  // ch1, side by side, each with the fused SGD of all_reduce_sgd; the launch's last block
  // advances step_ctr.  (Multi-rank tests drive the production kernel through this.)
  void all_reduce_pair(int ch0, int ch1, hipStream_t s, const SgdArgs& sgd, float* params, float* mbuf,
                       const ShadowSet& sh, int* step_ctr);
  // != 0: a barrier timed out (result invalid) - the first failed channel's error word
  // (xgmi_error_code: block, peer, barrier)
  unsigned error_flags() const;
  void set_timeout(double seconds) { timeout_s_ = seconds; }
  int rank() const { return rank_; }
  int world() const { return world_; }
  int channels() const { return (int)ch_.size(); }
  long data_numel() const { return data_numel_; }

 private:
  struct Channel {
    long off = 0, n = 0, slice = 0;
    int blocks = 1;
    bool oneshot = false;
    float* stage_local = nullptr;
    unsigned* sig_local = nullptr;
    float* stage[XGMI_MAX_RANKS] = {};
    unsigned* sig[XGMI_MAX_RANKS] = {};
  };
  int rank_, world_, device_;
  float* data_ = nullptr;
  long data_numel_ = 0;
  char* data_base_ = nullptr;
  long data_off_ = 0;
  float* data_peer_[XGMI_MAX_RANKS] = {};
  std::vector<Channel> ch_;
  std::vector<void*> opened_;
  bool imported_ = false;
  double timeout_s_ = XGMI_DEFAULT_TIMEOUT_S;
  struct PairArgs {  // all_reduce_pair: device copies of the argument pairs, one per content
    XgmiArgs host[2];
    XgmiArgs* dev = nullptr;
  };
  std::vector<PairArgs> pair_cache_;
  int* pair_done_ = nullptr;  // the pair launch's last-block count (zeroed before each launch)
};

// `world` virtual ranks of the all-reduce on ONE GPU in one process: every call is one launch
// (xgmi_allreduce_group) in which each rank's blocks run the production kernel body from
// arguments filled like XgmiComm's, against the other ranks' blocks of the same launch.  The
// arithmetic, index mapping and barrier protocol of every world size run deterministically in
// milliseconds (tests/test_xgmi_loopback_gpu.py); links, IPC mappings and skew between
// ranks' launches stay with the multi-process tests.  The caller owns every data and stage
// buffer (so a test can put guard bands round them) and keeps them alive.
class XgmiLoopback {
 public:
  static constexpr double kTimeoutS = 2.0;  // peers are co-resident: a correct barrier waits microseconds
  struct RankBuffers {  // one virtual rank's fused-SGD operands (see XgmiArgs)
    float* params = nullptr;
    float* mbuf = nullptr;
    ShadowSet sh{};
    int* step_ctr = nullptr;
  };
  XgmiLoopback(int world, int device);
  ~XgmiLoopback();
  XgmiLoopback(const XgmiLoopback&) = delete;
  XgmiLoopback& operator=(const XgmiLoopback&) = delete;
  void set_data(int rank, float* data, long numel);  // may be called again between calls
  // blocks: most blocks per rank (0: xgmi_blocks); world * blocks(channel) <= XGMI_GROUP_MAX_BLOCKS.
  // stage[r]: >= 2 * xgmi_stage_floats(n, world, oneshot) floats, 16-byte aligned
  int add_channel(long off, long n, bool oneshot, int blocks, const std::vector<float*>& stage,
                  const std::vector<long>& stage_numel);
  long slice(int channel) const { return ch_.at(channel).slice; }
  int blocks(int channel) const { return ch_.at(channel).blocks; }
  bool oneshot(int channel) const { return ch_.at(channel).oneshot; }
  int channels() const { return (int)ch_.size(); }
  int world() const { return world_; }
  long data_numel(int rank) const { return numel_[rank]; }
  void all_reduce(int channel, hipStream_t s, const SgdArgs& sgd, const std::vector<RankBuffers>& per_rank,
                  float scale, bool publish, float prescale, bool wt);
  unsigned error_flags() const;                      // the first non-zero error word of any rank
  unsigned seq(int channel, int rank, int blk) const;  // a block's call counter
  void set_timeout(double seconds) { timeout_s_ = seconds; }

 private:
  struct Channel {
    long off = 0, n = 0, slice = 0;
    int blocks = 1;
    bool oneshot = false;
    float* stage[XGMI_MAX_RANKS] = {};
    unsigned* sig[XGMI_MAX_RANKS] = {};
  };
  int world_, device_;
  float* data_[XGMI_MAX_RANKS] = {};
  long numel_[XGMI_MAX_RANKS] = {};
  std::vector<Channel> ch_;
  XgmiArgs* dev_args_ = nullptr;
  double timeout_s_ = kTimeoutS;
};

// ---------------------------------------------------------------- gradient reducer
// DDP gradient synchronisation for an arbitrary list of parameters (the module
// path).  Gradients live in one flat fp32 buffer cut into buckets; when the last
// gradient of a bucket is marked ready, an event is recorded on the compute
// stream, the comm stream waits for it and RCCL all-reduces the bucket, so
// communication of early buckets overlaps the rest of backward.  finalize()
// makes the compute stream wait for every bucket.  All of it is stream-ordered
// and therefore capturable into a hipGraph.
// comm == null with an XgmiComm (set_xgmi) reduces over the direct xGMI kernels only
// (e.g. ranks bootstrapped over gloo); world() comes from whichever data plane is set.
class Reducer {
 public:
  Reducer(std::shared_ptr<Comm> comm, float* flat_grad, std::vector<long> param_offsets,
          std::vector<long> param_numels, std::vector<int> param_bucket,
          std::vector<long> bucket_offsets, std::vector<long> bucket_numels, bool prescale);
  // bucket b all-reduced by xGMI channel channels[b] (its range must match the bucket)
  void set_xgmi(std::shared_ptr<XgmiComm> x, std::vector<int> channels);
  int world() const;
  ~Reducer();
  // grad_src == nullptr: gradient already written in place (bucket view)
  void mark_ready(int param, const float* grad_src, hipStream_t compute);
  void finalize(hipStream_t compute);
  void reset();
  int num_buckets() const { return (int)bucket_off_.size(); }
  long allreduce_calls() const { return calls_; }

 private:
  void launch_bucket(int b, hipStream_t compute);
  std::shared_ptr<Comm> comm_;
  std::shared_ptr<XgmiComm> xgmi_;
  std::vector<int> xch_;
  float* flat_;
  std::vector<long> poff_, pnum_;
  std::vector<int> pbucket_;
  std::vector<long> bucket_off_, bucket_num_;
  BucketState state_;
  std::vector<hipEvent_t> ready_, done_;
  hipStream_t comm_stream_ = nullptr;
  bool prescale_;
  long calls_ = 0;
};

// ---------------------------------------------------------------- fused SimpleCNN engine
struct EngineBuffers {
  // parameters / gradients: one flat fp32 buffer each (native layouts, see layers.py)
  float* params;
  float* grads;
  float* momentum;  // may be null (momentum == 0)
  long n_params;
  long off_w1, off_b1, off_w2, off_b2, off_wfc, off_bfc;
  // bf16 shadows
  bf16_t *w2_bf16, *w2t_bf16, *wfc_bf16, *wfc_frag;  // wfc_frag: FCFRAG order (conv2 fwd FC epilogue)
  // exact-fp32 engine (EngineConfig::f32): fp32 activations and the conv2 weight's
  // [tap][ci][co] fp32 copy (the data-gradient operand); the bf16 buffers are unused
  float *a2_f32 = nullptr, *dz2_f32 = nullptr, *w2t_f32 = nullptr;
  float* wfc_frag32 = nullptr;  // the fc weight in FCFRAG order, fp32 (the forward's fc operand)
  // activations / scratch (sized for max batch)
  bf16_t *a1, *a2, *dz2, *dz1;
  float *fc_part, *dlogits, *loss_rows, *loss_hist, *w2slab, *w1slab;
  int* step_ctr;
  unsigned char* xb;  // the step's batch, compact: u8 [max_batch][H*W] (fuse level 1)
  int* yb;            // its labels [max_batch]
  // in-launch hand-offs: [0, SYNC_RED_INTS) the fused conv backward's 8 arrival counters
  // (32 ints apart); level 3 and the one-stream xGMI chains: [SYNC_RED_INTS, + L3_FC_INTS)
  // the fc backward's last-block counter and, 8 / 16 / 24 ints in, the bucket all-reduce
  // roles' fc_done / red_done / xar_done counters (make_xar) - all of these zeroed by each
  // step's forward (C1Src::zero_i32); dist_mode 4: [L3_HEAD_OFF, + 2 * FWD_DZ_CNT_STRIDE) the
  // step head's two bucket-done counters (zeroed by the fc backward's last block).
  // sync_err: the wait-timeout word, sticky (0 = ok, RED_ERR = fused slab reduction,
  // FWD_DZ_ERR = level-3 forward's granule sweep, XAR_ERR = in-launch all-reduce,
  // HEAD_ERR = step head; launchers.h)
  int* sync_flags = nullptr;
  int* sync_err = nullptr;
  // data
  const unsigned char* images;  // u8 [N][H*W]
  const int* labels;            // i32 [N]
  const int* idx;               // i32 epoch index list (nullptr: images / labels already in epoch order)
  int n_idx, n_rows;            // bounds for the clamped batch gather
};

constexpr int L3_FC_INTS = 32;                          // [SYNC_RED_INTS, + 32): fc last-block counter
constexpr int L3_HEAD_OFF = SYNC_RED_INTS + L3_FC_INTS;  // dist_mode 4: the two bucket-done counters

// Gradient bucket of the engine's data plane: a [off, off + n) range of the flat gradient
// buffer.  Any plan works (DDP's bucket_cap_mb rule, sub-parameter chunks): a bucket is
// all-reduced as soon as every gradient in it is final - right after fc_bwd when it lies
// inside the fc parameters (overlapping the conv backward), after grad_reduce otherwise.
struct EngineBucket {
  long off, n;
};

class SimpleCNNEngine {
 public:
  SimpleCNNEngine(const EngineConfig& cfg, const EngineBuffers& buf, std::shared_ptr<Comm> comm,
                  std::vector<EngineBucket> buckets);
  ~SimpleCNNEngine();
  // eager launches of one full training step on the engine's compute stream
  void step(int batch, int batch_stride);
  void refresh_shadows();
  void set_lr(float lr) { cfg_.lr = lr; }
  // capture `nsteps` consecutive steps (batch = batch_stride = max_batch) into a graph
  void capture(int nsteps);
  void replay();
  bool has_graph() const { return graph_exec_ != nullptr; }
  int graph_steps() const { return graph_steps_; }
  void destroy_graph();
  hipStream_t stream() const { return cs_; }
  void synchronize();  // throws if an in-launch hand-off wait of a step timed out (sync_error)
  // in-launch wait-timeout word (EngineBuffers::sync_err: 0 = ok, RED_ERR, FWD_DZ_ERR,
  // XAR_ERR or HEAD_ERR); sticky
  int sync_error() const { return err_host_ ? __atomic_load_n(err_host_, __ATOMIC_ACQUIRE) : 0; }
  // whether a step of `batch` images runs the level-3 chain (fuse_level 3 and it applies)
  bool level3_active(int batch) { return plan(batch).l3; }
  // whether dist_mode 4's step head applies to a captured full-batch step
  bool overlap_active() { return plan(cfg_.max_batch).ov && pair_plan_ok_ && cfg_.pxt_fwd == 1; }
  // whether the last launched step reduced its weight-gradient slabs inside the conv
  // backward launch (false: separate grad_reduce kernel)
  bool last_fused_reduce() const { return last_fused_reduce_; }
  // whether the last launched step ran the level-3 chain (dZ2 in the forward, fc beside)
  bool last_level3() const { return last_level3_; }
  // ... and whether its fc weight gradient ran as a role of the conv backward launch
  bool last_fc_role() const { return last_fc_role_; }
  // ... and whether its bucket all-reduces ran inside the conv backward launch (dist_mode 2)
  bool last_xar() const { return last_xar_; }
  // ... or behind it in one launch for both buckets (dist_mode 3, xgmi_allreduce_pair)
  bool last_pair() const { return last_pair_; }
  // ... and whether its forward shared a launch with the previous step's pair (dist_mode 4)
  bool last_head() const { return last_head_; }
  // step-head launches (pair + next forward in one launch) in the captured graph
  int graph_heads() const { return graph_heads_; }
  void set_momentum_started(bool v) { momentum_started_ = v; }
  // bucket all-reduces over the direct xGMI kernel instead of RCCL: channels[b] serves
  // bucket b; set before capturing a graph
  void set_xgmi(std::shared_ptr<XgmiComm> x, std::vector<int> channels);
  int num_buckets() const { return (int)buckets_.size(); }
  int bucket_stage(int b) const { return stage_.at(b); }

 private:
  // parts of a step (dist_mode 4 splits steps inside a captured graph): the forward, the
  // backward, the bucket all-reduce pair; PART_HEAD = the forward merged with the PREVIOUS
  // step's pair (step_head_kernel)
  enum : unsigned { PART_FWD = 1, PART_BWD = 2, PART_AR = 4, PART_HEAD = 8, PART_ALL = 7 };
  void launch_step(int batch, int batch_stride, bool first_momentum_step, unsigned parts = PART_ALL);
  // the step on bf16 operands (T = bf16_t) or on exact fp32 operands (T = float)
  template <typename T>
  void launch_step_t(int batch, int batch_stride, bool first_momentum_step, unsigned parts);
  // the chain a step of `batch` images runs (step_plan.h: the only place that decides it)
  StepPlan plan(int batch);
  // every derived copy of the weights the step reads (a bucket's fused SGD refreshes the ones
  // inside its range): bf16 - conv2 plain, conv2 [tap][ci][co], fc fragment order and, with
  // plain_fc, the plain fc shadow; fp32 - the conv2 [tap][ci][co] and fc fragment-order copies
  ShadowSet shadow_set(bool plain_fc) const;
  // the blocks of a step, each filling one launcher struct (engine.cpp, in step order)
  C1Src make_c1src(int B, int stride, const StepPlan& pl) const;
  FwdDz make_fwd_dz(int B) const;
  FcBwdExtras make_fc_extras(int B, const StepPlan& pl, const SgdArgs& sa) const;
  SlabSet make_slabs(int B, const StepPlan& pl, const SgdArgs& sa) const;
  // PART_HEAD (bf16): the previous step's pair + this step's forward in one launch; false:
  // the merged grid does not fit - the pair ran alone and the caller launches the forward
  bool launch_step_head(int B, const SgdArgs& sa, const ShadowSet& sh, const C1Src& c1, const FwdDz& dzo);
  // enqueue the all-reduces of the buckets of `stage` (0: after fc_bwd, 1: after
  // grad_reduce) on the comm stream behind an event of the compute stream; with xGMI the
  // optimizer (+ the shadows in `sh`) runs inside each bucket's all-gather and the last
  // bucket of the step advances the step counter
  void launch_buckets(int stage, bool use_x, const SgdArgs& sa, float* M, const ShadowSet& sh);
  // compute stream waits for every launched stage
  void join_buckets();
  // the buckets of `stage` on stream s (no cross-stream ordering)
  void enqueue_buckets(int stage, bool use_x, hipStream_t s, const SgdArgs& sa, float* M, const ShadowSet& sh);
  // backward of a step whose forward is queued on cs_: the fc weight-gradient kernel `fc`
  // (may be empty: the fc role runs inside the conv backward), the conv backward `conv`
  // and, at world size > 1, the bucket all-reduces, ordered for the chain in use
  // (dist_mode 0 / 1); returns with every part of the step joined into cs_
  void schedule_backward(bool dist, bool fork, bool use_x, const std::function<void(hipStream_t)>& fc,
                         const std::function<void()>& conv, const SgdArgs& sa, float* M, const ShadowSet& sh);
  // dist_mode 2 with this bucket plan / data plane: the in-launch all-reduce's arguments for
  // this step (false: not applicable - the caller uses the bucket kernels)
  // the step head may defer a shadow of [off, off + n) to after the conv bucket's count
  bool late_shadow_ok(long off, long n) const;
  bool make_xar(BwdXar& xa, const SgdArgs& sa, float* M, const ShadowSet& sh);
  bool sync_ok_for_xar() const;
  EngineConfig cfg_;
  EngineBuffers b_;
  std::shared_ptr<Comm> comm_;
  std::shared_ptr<XgmiComm> xgmi_;
  std::vector<EngineBucket> buckets_;
  std::vector<int> stage_;  // 0: final after fc_bwd, 1: after grad_reduce
  std::vector<int> xch_;    // xGMI channel of each bucket
  int last_bucket_ = -1;    // the step's last collective (advances the step counter)
  bool stage_used_[2] = {false, false};
  hipStream_t cs_ = nullptr, ms_ = nullptr;
  hipEvent_t e_b0_, e_b1_, e_d0_, e_d1_, e_fwd_, e_fc_;
  std::vector<signed char> l3_fits_;  // per batch size: -1 unknown, 0 / 1
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t graph_exec_ = nullptr;
  int graph_steps_ = 0;
  bool momentum_started_ = false;
  bool last_fused_reduce_ = false;
  bool last_level3_ = false;
  bool last_fc_role_ = false;
  bool last_xar_ = false;
  bool last_pair_ = false;
  bool last_head_ = false;
  bool capturing_ = false;
  int graph_heads_ = 0;  // step-head launches in the captured graph (dist_mode 4)
  bool xar_plan_ok_ = false;  // set_xgmi: the bucket plan fits the in-launch all-reduce
  bool pair_plan_ok_ = false;  // ... and the one-launch pair of bucket kernels (dist_mode 3)
  struct XarArgs {
    XgmiArgs host[2];
    const XgmiArgs* dev = nullptr;
  };
  std::vector<XarArgs> xar_cache_;  // make_xar: device copies of the in-launch arguments
  hipStream_t xs_ = nullptr;        // ... and the stream their copies run on
  bool plain_stale_ = false;  // level-3 steps skipped the plain bf16 fc shadow
  int* err_host_ = nullptr;  // coherent host word behind b_.sync_err
  // level 3 (launchers.h FwdDz): the forward's partial-logit granules - [blocks][2][NO] 8-byte
  // {tag, float bits} words, an allocation of their own sized for max_batch at pxt_fwd 1,
  // zeroed once here - and the generation word the tags derive from (advanced once per step
  // by the fc backward; never restarted, unlike step_ctr, so no tag ever recurs)
  unsigned long long* gran_ = nullptr;
  unsigned* gen_ = nullptr;
};

}  // namespace ddp_amd
