// Host-only chain selection of the fused SimpleCNN step (no HIP, no RCCL, no torch): the
// engine's configuration and the one function that decides, from it and from a few facts
// the engine looks up, which chain a step of B images runs.  Kept free of device code so it
// is built and exercised under -fsanitize=address,undefined on the host
// (tests/native/test_step_plan.cpp).  engine.cpp reads the plan; it derives none of these
// booleans itself.
#pragma once

namespace ddp_amd {

struct EngineConfig {
  int max_batch, H, W, C1, C2, NO;
  int pxt_fwd, pxt_dgrad, wgrad_rows;
  int world, rank;
  float lr, momentum, dampening, weight_decay;
  int nesterov, maximize;
  int force_allreduce;  // run the bucket all-reduces even at world size 1 (tests)
  // 0: 8 kernels (a1 materialised, separate cross-entropy kernel)
  // 1: 6 kernels - conv1 recomputed inside conv2 fwd/dgrad/wgrad from the uint8
  //    images (a1 never touches HBM) and cross-entropy folded into fc_bwd
  //    (4 per step with the fused optimizer: conv fwd, fc_bwd, conv bwd, grad_reduce)
  // (2: a level-1 variant with fc_bwd and the conv backward in one launch - measured
  //    slower than level 1 and removed in round 4)
  // 3: the fc backward leaves the critical path - the conv forward computes dZ2 itself
  //    (FwdDz: per-image in-launch granule sweep, then dL and dZ2 from the fc weight fragments it
  //    holds) and the fc weight gradient + fused SGD (fc_bwd without dX, dL given) runs as
  //    a third role of the conv backward launch (single process, l3_fc_role: 2 kernels per
  //    step), or as a light kernel between the two (world size > 1: the fc bucket's
  //    all-reduce overlaps the conv backward).  Where every forward block fits on the
  //    GPU at once (conv3x3_fwd_dz_fits); otherwise the level-1 chain
  int fuse_level = 0;
  // level 3, single process: 1 = the fc weight gradient as a role of the conv backward
  // launch, on blocks after every conv block (the resident slots they leave free); 0 = as
  // its own kernel (what world size > 1 runs).  (Placements 2 / 3 - right after the dgrad
  // blocks, on the dgrad blocks - measured slower and were removed in round 4.)
  int l3_fc_role = 1;
  // 1: single-process steps apply SGD in the epilogues of fc_bwd / grad_reduce (no
  //    separate optimizer kernel); 0: always the flat SGD kernel (equivalence tests)
  int fuse_opt = 1;
  // level 1: 0 = the conv backward recomputes conv1 from the compact batch; 1 = the
  // forward also stores a1 (own pixels) and the dgrad role reads its ReLU mask from it;
  // 2 = the wgrad role reads a1 tiles too
  int store_a1 = 0;
  // 1: exact fp32 operands everywhere (v_mfma_f32_16x16x4_f32 conv2, fp32 fc, fp32
  //    activations), the reference's precision; needs fuse_level 1 or 3 and store_a1 0
  int f32 = 0;
  // 1: the conv backward launch also reduces the split-K slabs + fused SGD (no separate
  //    grad_reduce kernel; level >= 1, needs sync_flags) while its reducers fit half the
  //    launch's resident capacity; 2: the whole capacity when the step has no bucket
  //    all-reduce on another stream (single process: the exact-fp32 step fuses too);
  //    0: grad_reduce kernel
  int fuse_reduce = 1;
  // 2: the fused conv backward's wgrad role runs two blocks per slab row, one per half of
  //    conv2's input channels (bf16; bit-identical slabs); 1: one block per row
  int wgrad_split = 1;
  // world size > 1, level 3 - how the backward meets the bucket all-reduces:
  //  2 = in-launch (xGMI, at most one bucket per stage): the fc weight gradient runs as the
  //      conv backward's fc role, and role blocks at the head of that same launch all-reduce
  //      each bucket (+ fused SGD) as soon as its gradients are final (BwdXar) - 2 kernels
  //      per step, no cross-stream edge; falls back to the bucket kernels on the compute
  //      stream when a condition fails (RCCL: mode 1)
  //  1 = fork: fc_bwd and the fc buckets' all-reduces on the comm stream, forked after the
  //      forward beside the conv backward (a graph branch), the conv buckets' all-reduces
  //      behind the conv backward
  //  3 = one stream (xGMI, the default): the fc role inside the conv backward as on one GPU,
  //      then ONE launch running both buckets' all-reduces (+ fused SGD) side by side on
  //      full grids (xgmi_allreduce_pair; the bucket kernels one by one when the plan has
  //      more buckets per stage) - 3 kernels per step, no cross-stream edge.  Fastest
  //      measured (forced world 1: 639k img/s vs 444k in-launch, 416k fork;
  //      profiles/r5_dist/README.md): the in-launch roles get too few blocks, a graph
  //      branch costs two cross-stream edges
  //  0 = the round-4 order (fc_bwd in front of the conv backward, all-reduces on ms_)
  //  4 = the step head (xGMI, bf16 level 3, pxt_fwd 1): mode 3's chain, but in a captured
  //      graph the pair launch of step k also carries step k + 1's forward (conv3x3.hip
  //      step_head_kernel: the forward blocks wait for each bucket's all-reduce blocks only
  //      where they first read its parameters) - 2 launches per step instead of 3; the step
  //      counter advances in the conv backward's fc role.  Same bits as mode 3.  (fp32: mode
  //      3's chain.)
  int dist_mode = 3;
};

// What the engine looks up before it plans a step of B images.
struct StepFacts {
  bool xgmi = false;  // a direct xGMI data plane is set (SimpleCNNEngine::set_xgmi) ...
  int xgmi_world = 1;  // ... and its world size
  bool comm = false;  // an RCCL communicator was given ...
  int comm_world = 1;  // ... and its world size
  bool sync_flags = false, sync_err = false;  // EngineBuffers::sync_flags / sync_err present
  // every block of a level-3 forward of B images is resident at once (conv3x3_fwd_dz_fits),
  // at the SimpleCNN widths C1 == 32, C2 == 64
  bool l3_fits = false;
  bool fc_role_ok = false;   // conv3x3_bwd_fc_role_ok: the conv backward can take the fc role
  bool xar_plan_ok = false;  // the bucket plan fits the in-launch all-reduce (set_xgmi)
};

struct StepPlan {
  bool use_x;  // the buckets are all-reduced by the direct xGMI kernels (SGD fused into them)
  bool dist;   // the step has bucket all-reduces at all (xGMI or RCCL)
  bool f1;     // level >= 1: conv1 recomputed, cross-entropy off its own kernel
  bool l3;     // the level-3 chain: the forward also writes dL and dZ2
  bool fred;   // the slab reduction runs inside the conv backward launch (when it fits)
  // dist_mode 3 / 4 on any chain from level 1 up (the same-GPU multi-rank rehearsals run
  // level 1): one stream, both buckets in one launch behind the conv backward
  bool pair_mode;
  // level 3 over xGMI with the fc role allowed at world size > 1: dist_mode 2 (its gradient
  // all-reduced in-launch) and dist_mode 3 / 4
  bool xar_mode;
  // the one-stream chains: fc weight gradient (role or kernel) -> conv backward -> the bucket
  // all-reduces, all on the compute stream.  The engine tests this first: only the other
  // chains go through schedule_backward, which alone reads `fork`
  bool one_stream;
  // the fc weight gradient runs as a third role of the conv backward launch: single process
  // (2 kernels per step) or a one-stream xGMI chain; otherwise as its own light kernel
  bool fc_role;
  // dist_mode 4 (the step head, bf16): mode 3's chain, but the step counter advances in the
  // conv backward's fc role (after it read the loss index) instead of the pair launch, so
  // that the pair launch can carry the NEXT step's forward (which reads the counter)
  bool ov;
  // single-process steps: no all-reduce separates a gradient from its update, so the
  // optimizer runs in the epilogues of the kernels that finish each gradient
  bool fopt;
  bool fork;        // dist_mode 1: fc_bwd + the fc buckets on the comm stream beside the conv backward
  bool xar_wanted;  // dist_mode 2: ask for the in-launch all-reduce (make_xar has the last word)
};

inline StepPlan plan_step(const EngineConfig& c, const StepFacts& f, int B) {
  StepPlan p{};
  p.use_x = f.xgmi && (f.xgmi_world > 1 || c.force_allreduce);
  p.dist = p.use_x || (f.comm && (f.comm_world > 1 || c.force_allreduce));
  p.f1 = c.fuse_level >= 1;
  p.l3 = c.fuse_level >= 3 && f.sync_flags && f.sync_err && B > 0 && B <= c.max_batch && f.l3_fits;
  p.fred = p.f1 && c.fuse_reduce && f.sync_flags;
  p.pair_mode = p.dist && p.use_x && p.f1 && c.dist_mode >= 3 && f.sync_flags && f.sync_err;
  p.xar_mode = p.dist && p.use_x && p.l3 && ((c.dist_mode == 2 && f.xar_plan_ok) || c.dist_mode >= 3);
  p.one_stream = p.xar_mode || p.pair_mode;
  p.fc_role = p.l3 && (!p.dist || p.xar_mode) && c.l3_fc_role && f.fc_role_ok;
  p.ov = !c.f32 && p.dist && p.use_x && p.l3 && p.fc_role && c.dist_mode == 4;
  p.fopt = !p.dist && c.fuse_opt;
  p.fork = p.dist && p.l3 && c.dist_mode == 1;
  p.xar_wanted = p.xar_mode && c.dist_mode == 2 && p.fc_role && p.fred;
  return p;
}

}  // namespace ddp_amd
