// rtj_host_switches.h — every environment switch of the host layer, read in one place each.  No HIP types: a plain host
// program can include this header (tests/test_plan_switches_cpu.py does, and prints the table below).
//
// Tuning knobs of the product (launch sizes, group sizes, which index runs) are read with getenv; switches that only
// exist to take measurements — the ones that leave work out (wrong or no pictures) and the A/B forms that were measured
// slower and are kept for the record — are read through exp_env(), which a product build compiles to "not set": they
// exist in builds with -DMIRTJ_EXPERIMENTS only (tools/ builds those next to the product).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace mirtj {

static inline const char* exp_env(const char* name) {
#ifdef MIRTJ_EXPERIMENTS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// Who makes the plan decides which switches it honours (DESIGN.md has the same table):
//   batch (mi_rtj_plan_create)    MI_RTJ_INDEX, _EMIT, _SPEC, _SPEC_RUN, _DEC_SLOTS, _ROTATE, _SERIAL_MIN, _SPLIT, _OVERLAP
//   one packet (mi_rtj_decode*)   MI_RTJ_INDEX, _EMIT, _SPEC, _SPEC_RUN; the rest at their defaults
//   session slot, session group   MI_RTJ_INDEX, _EMIT; no speculation (one or a handful of packets per launch: a lone
//                                 walker takes longer than all of the exact index); the rest at their defaults
enum PlanKind { kPlanBatch = 0, kPlanOnePacket, kPlanSessionSlot, kPlanSessionGroup };

struct PlanSwitches {
  bool serial_index = false;   // MI_RTJ_INDEX=serial: one wave per packet (A/B baseline)
  bool emit_walk = false;      // MI_RTJ_EMIT=walk: per-chunk re-walk instead of the length tables
  int spec_mode = -1;          // MI_RTJ_SPEC: 0 never, 1 / 3 / 4 always with the short / long / very long lead (no policy),
                               // 2 whatever the batch size, otherwise by batch size
  int spec_run = 0;            // MI_RTJ_SPEC_RUN (A/B, tests): 1 .. 4 = chunks a walker of the short lead walks behind one lead,
                               // whatever the launch's size; otherwise by the number of chunks (spec_run_length())
  uint32_t dec_slots = 0;      // MI_RTJ_DEC_SLOTS (A/B): k_decode waves per part, 0 = decode_slots()
  int rotate = -1;             // MI_RTJ_ROTATE: 1 / 0 = a k_decode wave takes all three parts of its groups / one part; -1 = by batch size
  uint32_t serial_min = 4096;  // MI_RTJ_SERIAL_MIN: to-do lists from this many packets on go to the serial walker (0: never)
  int split = -1;              // MI_RTJ_SPLIT (A/B): 0 = batches always run k_decode<true, false>, 1 = always k_decode_split;
                               // otherwise the plan's policy decides on the device
  bool overlap_set = false;    // MI_RTJ_OVERLAP given: 1 = always, 2 = by the decode policy's mode word (tests, on small
  int overlap = 0;             // plans), anything else = never; not given: by the plan's size
};

static inline PlanSwitches plan_switches_from_env(PlanKind kind) {
  PlanSwitches s;
  const char* v = getenv("MI_RTJ_INDEX");
  s.serial_index = v && strcmp(v, "serial") == 0;
  v = getenv("MI_RTJ_EMIT");
  s.emit_walk = v && strcmp(v, "walk") == 0;
  if (kind == kPlanSessionSlot || kind == kPlanSessionGroup) {
    s.spec_mode = 0;
    return s;
  }
  if ((v = getenv("MI_RTJ_SPEC"))) s.spec_mode = atoi(v);
  if ((v = getenv("MI_RTJ_SPEC_RUN"))) s.spec_run = atoi(v);
  if (kind != kPlanBatch) return s;
  if ((v = getenv("MI_RTJ_DEC_SLOTS"))) s.dec_slots = (uint32_t)atoi(v);
  if ((v = getenv("MI_RTJ_ROTATE"))) s.rotate = atoi(v) != 0;
  if ((v = getenv("MI_RTJ_SERIAL_MIN"))) s.serial_min = (uint32_t)atoi(v);
  if ((v = getenv("MI_RTJ_SPLIT"))) s.split = atoi(v) != 0;
  if ((v = getenv("MI_RTJ_OVERLAP"))) {
    s.overlap_set = true;
    s.overlap = atoi(v);
  }
  return s;
}

// The experiment switches of a launch (timing builds only; tests/test_gpu_launch_shapes.py changes them between the
// launches of one process, so they are read at every launch — a product build reads nothing).
struct LaunchExperiments {
  uint32_t luma_waves = 0, chroma_waves = 0;  // MI_RTJ_LUMA_WAVES / MI_RTJ_CHROMA_WAVES: 0 = as computed
  uint32_t xcd_rot = 0;                       // MI_RTJ_XCD_ROT
  int split_only = 0;                         // MI_RTJ_SPLIT_ONLY (wrong pictures): 1 the luma waves alone, else the chroma waves alone
};

static inline LaunchExperiments launch_experiments_from_env(uint32_t xcd_rot_default) {
  LaunchExperiments x;
  x.xcd_rot = xcd_rot_default;
  if (const char* e = exp_env("MI_RTJ_LUMA_WAVES")) x.luma_waves = (uint32_t)atoi(e);
  if (const char* e = exp_env("MI_RTJ_CHROMA_WAVES")) x.chroma_waves = (uint32_t)atoi(e);
  if (const char* e = exp_env("MI_RTJ_XCD_ROT")) x.xcd_rot = (uint32_t)atoi(e);
  if (const char* e = exp_env("MI_RTJ_SPLIT_ONLY")) x.split_only = atoi(e) == 1 ? 1 : 2;
  return x;
}

// A session's own switches (mi_rtj_pipe_create), read once per session.
struct PipeSwitches {
  int out_streams = 2;     // MI_RTJ_OUT_STREAMS=1 (A/B): one copy-out stream
  int out_kernel = 0;      // MI_RTJ_OUT_KERNEL: the copy kernel's grid (workgroups of 256); 0 = the copy engine
  int exp_skip = 0;        // MI_RTJ_EXP_SKIP (wrong pictures): 1 no copy out, 2 no kernels, 4 no copy in
  bool stats = false;      // MI_RTJ_PIPE_STATS=1
  int wait_mode = 0;       // MI_RTJ_WAIT=query (A/B): poll instead of blocking inside the runtime
  bool out_group_set = false, idx_group_set = false;
  int out_group = 0;       // MI_RTJ_OUT_GROUP = 1 / 2 / 4; not given: by the depth
  int idx_group = 0;       // MI_RTJ_IDX_GROUP = 1 / 2 / 4; not given: the copy group
  bool threaded = false;   // MI_RTJ_PIPE_THREAD=1 (A/B): HIP calls on a worker thread
  bool stream_prio = true; // MI_RTJ_STREAM_PRIO=0 (A/B): every stream at the default priority
  bool idx_stream = false; // MI_RTJ_IDX_STREAM=1 (A/B, slower): index kernels on a stream of their own
};

static inline PipeSwitches pipe_switches_from_env() {
  PipeSwitches s;
  const char* v = exp_env("MI_RTJ_OUT_STREAMS");
  s.out_streams = v && atoi(v) == 1 ? 1 : 2;
  if ((v = exp_env("MI_RTJ_OUT_KERNEL"))) s.out_kernel = atoi(v);
  if ((v = exp_env("MI_RTJ_EXP_SKIP"))) s.exp_skip = atoi(v);
  v = getenv("MI_RTJ_PIPE_STATS");
  s.stats = v && atoi(v) != 0;
  v = exp_env("MI_RTJ_WAIT");
  s.wait_mode = v && strcmp(v, "query") == 0 ? 1 : 0;
  if ((v = getenv("MI_RTJ_OUT_GROUP"))) s.out_group_set = true, s.out_group = atoi(v);
  if ((v = getenv("MI_RTJ_IDX_GROUP"))) s.idx_group_set = true, s.idx_group = atoi(v);
  v = exp_env("MI_RTJ_PIPE_THREAD");
  s.threaded = v && atoi(v) != 0;
  v = getenv("MI_RTJ_STREAM_PRIO");
  s.stream_prio = !v || atoi(v) != 0;
  v = exp_env("MI_RTJ_IDX_STREAM");
  s.idx_stream = v && atoi(v) != 0;
  return s;
}

}  // namespace mirtj
