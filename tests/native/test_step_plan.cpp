// Host-only unit test of the fused step's chain selection (csrc/runtime/step_plan.h), built
// with -fsanitize=address,undefined by tests/test_native_host.py.  The expected plans are
// written out by hand from the table in step_plan.h; the sweep checks what the engine relies
// on, for every combination of the inputs.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "runtime/step_plan.h"

using ddp_amd::EngineConfig;
using ddp_amd::plan_step;
using ddp_amd::StepFacts;
using ddp_amd::StepPlan;

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

static const char* const kNames[] = {"use_x", "dist", "f1", "l3", "fred", "pair_mode", "xar_mode",
                                     "one_stream", "fc_role", "ov", "fopt", "fork", "xar_wanted"};
constexpr int kFields = sizeof(kNames) / sizeof(kNames[0]);

static void fields(const StepPlan& p, bool* out) {
  const bool v[kFields] = {p.use_x, p.dist, p.f1, p.l3, p.fred, p.pair_mode, p.xar_mode,
                           p.one_stream, p.fc_role, p.ov, p.fopt, p.fork, p.xar_wanted};
  for (int i = 0; i < kFields; ++i) out[i] = v[i];
}

// `want`: the names of the fields that are set, separated by blanks; every other field is clear
static void expect(const char* what, const StepPlan& got, const char* want) {
  bool g[kFields];
  fields(got, g);
  const std::string w = std::string(" ") + want + " ";
  for (int i = 0; i < kFields; ++i) {
    const bool e = w.find(std::string(" ") + kNames[i] + " ") != std::string::npos;
    if (g[i] != e) {
      std::fprintf(stderr, "%s: %s is %d, expected %d\n", what, kNames[i], (int)g[i], (int)e);
      std::exit(1);
    }
  }
}

static EngineConfig base_config() {
  EngineConfig c{};
  c.max_batch = 32;
  c.H = c.W = 28;
  c.C1 = 32;
  c.C2 = 64;
  c.NO = 10;
  c.pxt_fwd = c.pxt_dgrad = 2;
  c.wgrad_rows = 4;
  c.world = 1;
  c.fuse_level = 3;
  c.l3_fc_role = 1;
  c.fuse_opt = 1;
  c.fuse_reduce = 1;
  c.wgrad_split = 2;
  c.dist_mode = 3;
  return c;
}

static StepFacts base_facts() {
  StepFacts f;
  f.sync_flags = f.sync_err = true;
  f.l3_fits = f.fc_role_ok = f.xar_plan_ok = true;
  return f;
}

static void named_plans() {
  const int B = 32;
  {  // one GPU
    EngineConfig c = base_config();
    StepFacts f = base_facts();
    expect("one GPU, bf16, level 3", plan_step(c, f, B), "f1 l3 fred fc_role fopt");
    c.f32 = 1;
    c.fuse_reduce = 0;
    expect("one GPU, fp32, fuse_reduce 0", plan_step(c, f, B), "f1 l3 fc_role fopt");
    c = base_config();
    c.fuse_opt = 0;
    expect("one GPU, flat SGD kernel", plan_step(c, f, B), "f1 l3 fred fc_role");
    c = base_config();
    c.l3_fc_role = 0;
    expect("one GPU, fc_bwd as its own kernel", plan_step(c, f, B), "f1 l3 fred fopt");
    // an RCCL communicator / an xGMI plane of one rank, not forced: still the local chain
    c = base_config();
    f.comm = f.xgmi = true;
    expect("world 1, not forced", plan_step(c, f, B), "f1 l3 fred fc_role fopt");
  }
  {  // xGMI, world 1 with the all-reduces forced, and a real world of 8
    for (int world : {1, 8}) {
      EngineConfig c = base_config();
      StepFacts f = base_facts();
      f.xgmi = true;
      f.xgmi_world = world;
      c.force_allreduce = world == 1;
      c.dist_mode = 0;
      expect("xgmi mode 0", plan_step(c, f, B), "use_x dist f1 l3 fred");
      c.dist_mode = 1;
      expect("xgmi mode 1", plan_step(c, f, B), "use_x dist f1 l3 fred fork");
      c.dist_mode = 2;
      expect("xgmi mode 2", plan_step(c, f, B), "use_x dist f1 l3 fred xar_mode one_stream fc_role xar_wanted");
      f.xar_plan_ok = false;
      expect("xgmi mode 2, plan not ok", plan_step(c, f, B), "use_x dist f1 l3 fred");
      c.dist_mode = 3;  // (the pair does not need the in-launch plan)
      expect("xgmi mode 3", plan_step(c, f, B), "use_x dist f1 l3 fred pair_mode xar_mode one_stream fc_role");
      f.xar_plan_ok = true;
      expect("xgmi mode 3", plan_step(c, f, B), "use_x dist f1 l3 fred pair_mode xar_mode one_stream fc_role");
      c.dist_mode = 4;
      expect("xgmi mode 4 bf16", plan_step(c, f, B),
             "use_x dist f1 l3 fred pair_mode xar_mode one_stream fc_role ov");
      c.f32 = 1;
      expect("xgmi mode 4 fp32", plan_step(c, f, B), "use_x dist f1 l3 fred pair_mode xar_mode one_stream fc_role");
      c.f32 = 0;
      c.l3_fc_role = 0;  // no fc role: no step head, the in-launch all-reduce is not asked for
      expect("xgmi mode 4, no fc role", plan_step(c, f, B), "use_x dist f1 l3 fred pair_mode xar_mode one_stream");
      c.dist_mode = 2;
      expect("xgmi mode 2, no fc role", plan_step(c, f, B), "use_x dist f1 l3 fred xar_mode one_stream");
    }
  }
  {  // RCCL only
    for (int mode = 0; mode <= 4; ++mode) {
      EngineConfig c = base_config();
      StepFacts f = base_facts();
      f.comm = true;
      f.comm_world = 2;
      c.dist_mode = mode;
      expect("rccl", plan_step(c, f, B), mode == 1 ? "dist f1 l3 fred fork" : "dist f1 l3 fred");
      c.f32 = 1;
      expect("rccl fp32", plan_step(c, f, B), mode == 1 ? "dist f1 l3 fred fork" : "dist f1 l3 fred");
    }
  }
  {  // level 3 asked for, but it does not apply: the level-1 plan
    EngineConfig c = base_config();
    StepFacts f = base_facts();
    f.l3_fits = false;
    expect("level 3 does not fit", plan_step(c, f, B), "f1 fred fopt");
    f = base_facts();
    f.sync_err = false;
    expect("no sync_err", plan_step(c, f, B), "f1 fred fopt");
    f = base_facts();
    expect("batch 0", plan_step(c, f, 0), "f1 fred fopt");
    expect("batch > max_batch", plan_step(c, f, 33), "f1 fred fopt");
    expect("ragged batch", plan_step(c, f, 8), "f1 l3 fred fc_role fopt");
    f.sync_flags = false;
    expect("no sync_flags", plan_step(c, f, B), "f1 fopt");
    c.fuse_level = 1;
    f = base_facts();
    expect("level 1", plan_step(c, f, B), "f1 fred fopt");
    // level 1 over xGMI: mode 3 / 4 still run one stream with the pair launch; the fc
    // weight gradient is fc_bwd (no role)
    f.xgmi = true;
    c.force_allreduce = 1;
    expect("level 1, xgmi mode 3", plan_step(c, f, B), "use_x dist f1 fred pair_mode one_stream");
    c.dist_mode = 4;
    expect("level 1, xgmi mode 4", plan_step(c, f, B), "use_x dist f1 fred pair_mode one_stream");
    c.dist_mode = 1;
    expect("level 1, xgmi mode 1", plan_step(c, f, B), "use_x dist f1 fred");
    c.dist_mode = 3;
    c.fuse_level = 3;
    f.l3_fits = false;
    expect("level 3 does not fit, xgmi mode 3", plan_step(c, f, B), "use_x dist f1 fred pair_mode one_stream");
    f.l3_fits = true;
    f.sync_err = false;
    expect("no sync_err, xgmi mode 3", plan_step(c, f, B), "use_x dist f1 fred");
  }
  {  // level 0: nothing but dist, use_x, fopt
    EngineConfig c = base_config();
    StepFacts f = base_facts();
    c.fuse_level = 0;
    expect("level 0", plan_step(c, f, B), "fopt");
    f.comm = true;
    f.comm_world = 4;
    expect("level 0, rccl", plan_step(c, f, B), "dist");
    f.xgmi = true;
    f.xgmi_world = 4;
    for (int mode = 0; mode <= 4; ++mode) {
      c.dist_mode = mode;
      expect("level 0, xgmi", plan_step(c, f, B), "use_x dist");
    }
  }
}

// every combination of the inputs; returns the number of plans checked
static long sweep() {
  long n = 0;
  int seen[kFields] = {};
  for (int bits = 0; bits < (1 << 13); ++bits) {
    auto bit = [&](int i) { return ((bits >> i) & 1) != 0; };
    EngineConfig c = base_config();
    StepFacts f;
    c.f32 = bit(0);
    c.force_allreduce = bit(1);
    c.l3_fc_role = bit(2);
    c.fuse_opt = bit(3);
    f.xgmi = bit(4);
    f.xgmi_world = bit(5) ? 8 : 1;
    f.comm = bit(6);
    f.comm_world = bit(7) ? 8 : 1;
    f.sync_flags = bit(8);
    f.sync_err = bit(9);
    f.l3_fits = bit(10);
    f.fc_role_ok = bit(11);
    f.xar_plan_ok = bit(12);
    for (int mode = 0; mode <= 4; ++mode)
      for (int level : {0, 1, 3})
        for (int red = 0; red <= 2; ++red)
          for (int B : {0, 8, 32, 33}) {
            c.dist_mode = mode;
            c.fuse_level = level;
            c.fuse_reduce = red;
            const StepPlan p = plan_step(c, f, B);
            ++n;
            bool g[kFields];
            fields(p, g);
            for (int i = 0; i < kFields; ++i) seen[i] += g[i];
            // the invariants launch_step / capture() rely on
            if (p.ov) CHECK(p.fc_role && p.one_stream && !c.f32);
            if (p.xar_wanted) CHECK(p.fc_role && p.fred);
            if (p.fc_role) CHECK(p.l3);
            if (p.fopt) CHECK(!p.dist);
            // inputs the plan must respect
            if (p.use_x) CHECK(p.dist && f.xgmi);
            if (!f.xgmi) CHECK(!p.pair_mode && !p.xar_mode && !p.ov && !p.xar_wanted);
            if (p.dist && !p.use_x) CHECK(!p.fc_role && !p.one_stream);  // RCCL: fc_bwd is its own kernel
            if (p.l3) CHECK(p.f1 && level >= 3 && B > 0 && B <= c.max_batch && f.l3_fits && f.sync_flags && f.sync_err);
            if (p.fred) CHECK(p.f1 && red != 0 && f.sync_flags);
            if (level == 0) CHECK(!p.f1 && !p.l3 && !p.fred && !p.one_stream && !p.fc_role && !p.fork);
            // the hand-off counters the one-stream chains and the fused reduction count in exist
            if (p.one_stream || p.fred || p.l3) CHECK(f.sync_flags);
            if (p.one_stream) CHECK(f.sync_err);
            // one_stream comes first: the engine tests it before it hands the backward to
            // schedule_backward (which alone reads `fork`), so a one-stream chain is an xGMI
            // chain on the compute stream whatever `fork` says
            CHECK(p.one_stream == (p.xar_mode || p.pair_mode));
            if (p.one_stream) CHECK(p.dist && p.use_x && p.f1);
            if (p.fork) CHECK(p.dist && p.l3 && mode == 1);
            // the dist_mode each chain belongs to
            if (p.pair_mode) CHECK(mode >= 3);
            if (p.xar_mode) CHECK(mode >= 2 && p.l3);
            if (p.xar_wanted) CHECK(mode == 2 && f.xar_plan_ok);
            if (p.ov) CHECK(mode == 4 && p.pair_mode && p.xar_mode);
          }
  }
  for (int i = 0; i < kFields; ++i) CHECK(seen[i] > 0);  // (no field is dead in the sweep)
  return n;
}

int main() {
  named_plans();
  const long n = sweep();
  std::printf("step plan: %ld plans swept, all checks passed\n", n);
  return 0;
}
