// rtj_host_stages.h — the stages of a plan's launch, in the order plan_launch() (mi_rtjpeg.hip) calls them.  plan_launch
// keeps everything that sizes a grid; a stage gets its grids as arguments and queues kernels, events and waits.
// Included by mi_rtjpeg.hip behind the definitions of mi_rtj_ctx and mi_rtj_plan.
#pragma once

namespace {

#define STAGE_CHK(call)                              \
  do {                                               \
    const int rc_ = (call);                          \
    if (rc_ != MI_RTJ_OK) return rc_;                \
  } while (0)

// a timing event of the plan's: it lives until profiling is switched or the plan goes
int timing_event(mi_rtj_plan* p, hipEvent_t* e) {
  Event ev;
  HIPCHK(p->ctx, hipEventCreate(&ev.p));
  *e = ev;
  p->timing.push_back(std::move(ev));
  return MI_RTJ_OK;
}

// While profiling: one event after every kernel; a kernel's start is its predecessor's end (they run back to back on one
// stream), so a launch costs one event record per kernel instead of two.  Without profiling begin / end do nothing.
struct KernelClock {
  mi_rtj_plan* p;
  hipStream_t cur;
  hipEvent_t prev = nullptr;  // the end of the kernel queued last, while that is this kernel's start
  Timed t;

  int begin() {
    if (!p->profile) return MI_RTJ_OK;
    t = Timed();
    if (prev) {
      t.a = prev;
      return MI_RTJ_OK;
    }
    STAGE_CHK(timing_event(p, &t.a));
    HIPCHK(p->ctx, hipEventRecord(t.a, cur));
    return MI_RTJ_OK;
  }
  int end(int k) {
    if (!p->profile) return MI_RTJ_OK;
    STAGE_CHK(timing_event(p, &t.b));
    HIPCHK(p->ctx, hipEventRecord(t.b, cur));
    p->ev[k].push_back(t);
    prev = t.b;
    return MI_RTJ_OK;
  }
};

// what the stages of one launch share
struct Launch {
  mi_rtj_plan* p;
  mi_rtj_ctx* c;
  const uint8_t* st;       // the packets' stream
  bool ov = false;         // this launch builds its index on the plan's own stream, next to the transform before it
  hipStream_t ds, is;      // the transform's stream (the instance's) and the index kernels'
  uint32_t* blk = nullptr; // the block index this launch writes and reads
  KernelClock clk;
  // the speculative index leaves these to the exact one: the packets it could not prove (count, list) and the policy's state
  const uint32_t *todo = nullptr, *ntodo = nullptr;
  uint32_t* state = nullptr;

  Launch(mi_rtj_plan* plan, const uint8_t* stream)
      : p(plan), c(plan->ctx), st(stream), ds(plan->ctx->stream), is(plan->ctx->stream), clk{plan, plan->ctx->stream} {}
};

// ---- dispatch on what the kernels are templates of ----
void launch_index_fmt(int fmt, dim3 grid, hipStream_t s, const FrameDev* fr, uint32_t n, const uint8_t* st, const QTab* lut, uint32_t* blk) {
  if (fmt == MI_RTJ_FMT_YUV422) hipLaunchKernelGGL(k_index_fmt<kFmtYUV422>, grid, dim3(64), 0, s, fr, n, st, lut, blk);
  else hipLaunchKernelGGL(k_index_fmt<kFmtGrey>, grid, dim3(64), 0, s, fr, n, st, lut, blk);
}
void launch_decode_fmt(int fmt, dim3 grid, hipStream_t s, const FrameDev* fr, const uint8_t* st, const QTab* lut, const uint32_t* blk, uint8_t* out) {
  if (fmt == MI_RTJ_FMT_YUV422) hipLaunchKernelGGL(k_decode_fmt<kFmtYUV422>, grid, dim3(kDecThreads), 0, s, fr, st, lut, blk, out);
  else hipLaunchKernelGGL(k_decode_fmt<kFmtGrey>, grid, dim3(kDecThreads), 0, s, fr, st, lut, blk, out);
}

// The walkers zero the launch's lists themselves (SpecReset).  With a policy ONE dispatch runs the form the policy's
// state names (or returns at once while the speculation is paused); without (MI_RTJ_SPEC = 1 / 3 / 4: tests) the form
// asked for.
// (a plain function, not a template: the kernels are instantiated where they are named, in this order)
struct WalkArgs {
  const FrameDev* frames;
  const SpecChunkDev* chunks;
  uint32_t total;
  const uint8_t* stream;
  const QTab* lut;
  uint32_t *recbits, *nrec, *wstart;
  uint2* hand;
  SpecReset rs;
  SpecRunArgs ra;  // a plan with runs (ra.runs): the short lead walks a lane per run, rtj_spec_kernels.h
};
#define WALK(kernel, ...) \
  hipLaunchKernelGGL(kernel, grid, dim3(64), 0, s, a.frames, a.chunks, a.total, a.stream, a.lut, a.recbits, a.nrec, a.wstart, a.hand, a.rs, a.ra, ##__VA_ARGS__)
void launch_spec_walk(bool two_types, int spec_mode, uint32_t* state, dim3 grid, hipStream_t s, const WalkArgs& a) {
  const bool runs = a.ra.runs != nullptr;
  if (state) {
    if (!two_types) {
      if (runs) WALK((k_spec_walk_any<false, true>), state);
      else WALK((k_spec_walk_any<false>), state);
    } else {
      if (runs) WALK((k_spec_walk_any<true, true>), state);
      else WALK((k_spec_walk_any<true>), state);
    }
  } else if (runs) {  // (forced, MI_RTJ_SPEC=1 with MI_RTJ_SPEC_RUN: the short lead)
    if (!two_types) WALK((k_spec_walk<false, kSpecLead, true>));
    else WALK((k_spec_walk<true, kSpecLead, true>));
  } else if (!two_types) {
    if (spec_mode == 1) WALK((k_spec_walk<false, kSpecLead>));
    if (spec_mode == 3) WALK((k_spec_walk<false, kSpecLeadLong>));
    if (spec_mode == 4) WALK((k_spec_walk<false, kSpecLeadVery>));
  } else {
    if (spec_mode == 1) WALK((k_spec_walk<true, kSpecLead>));
    if (spec_mode == 3) WALK((k_spec_walk<true, kSpecLeadLong>));
    if (spec_mode == 4) WALK((k_spec_walk<true, kSpecLeadVery>));
  }
}
#undef WALK

struct RunGrids {
  dim3 mask, carry, copy;
  uint32_t items, copy_threads;
};
int stage_runs(Launch& L, bool runs, const RunGrids& g, uint8_t* out);

// ---- a 4:2:2 or greyscale plan: kernels back to back on the instance's stream (rtj_format_kernels.h) — the serial
// index, a wave per packet (MI_RTJ_K_EMIT), then the transform (MI_RTJ_K_DECODE), then phase 2 of a plan with runs
// (mi_rtj_plan_set_runs_fmt), which reads the index this launch wrote.  No speculative or chunk-parallel index, no
// second stream.
int launch_fmt(Launch& L, dim3 igrid, dim3 dgrid, bool runs, const RunGrids& rg, uint8_t* out) {
  mi_rtj_plan* p = L.p;
  L.c->input_dirty = false;  // (everything runs on the instance's stream)
  L.blk = p->blkoff;
  STAGE_CHK(L.clk.begin());
  launch_index_fmt(p->fmt, igrid, L.ds, p->d_frames, (uint32_t)p->n, L.st, L.c->d_lut, L.blk);
  STAGE_CHK(L.clk.end(MI_RTJ_K_EMIT));
  STAGE_CHK(L.clk.begin());
  launch_decode_fmt(p->fmt, dgrid, L.ds, p->d_frames, L.st, L.c->d_lut, L.blk, out);
  STAGE_CHK(L.clk.end(MI_RTJ_K_DECODE));
  STAGE_CHK(stage_runs(L, runs, rg, out));
  p->runs_ran = runs;
  HIPCHK(L.c, hipGetLastError());
  p->ov.last = 0;
  p->launches++;
  return MI_RTJ_OK;
}

// ---- stage 1: which streams and which index, and what they have to wait for ----
// The index kernels run on `is`, k_decode on the instance's stream.  Plans have them equal; a session gives its slots
// an index stream of their own (p->idx_stream), so that the index of packet i + 1 is built while packet i — whose
// picture the unchanged blocks of i + 1 come from — is still being transformed.
int launch_open(Launch& L, int what) {
  mi_rtj_plan* p = L.p;
  mi_rtj_ctx* c = L.c;
  L.ov = p->ov.on;
  if (!L.ov && p->ov.dyn && what == kLaunchAll && p->split.h_mode_seen &&
      *(volatile uint32_t*)p->split.h_mode_seen.p == (uint32_t)kDecModeClassic) {
    L.ov = true;  // (the second index and the stream were made with the plan: nothing is allocated on the launch path)
  }
  L.is = L.ov && !p->idx_stream ? p->ov.own_idx : p->idx_stream ? p->idx_stream : c->stream;
  L.clk.cur = L.is;
  // (a launch that overlaps behind one that did not: whatever the instance's stream still has queued — the last launch's
  // transform reading the first index, the plan's descriptors on their way — comes first)
  if (L.is != L.ds && (c->input_dirty || (L.ov && !p->ov.on && !p->ov.last_overlapped))) {  // something queued on the instance's stream may still be writing the packets
    if (!c->e_input) HIPCHK(c, hipEventCreateWithFlags(&c->e_input.p, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->e_input, L.ds));
    HIPCHK(c, hipStreamWaitEvent(L.is, c->e_input, 0));
  }
  c->input_dirty = false;
  L.blk = L.ov && p->ov.flip ? p->ov.blkoff_b.p : p->blkoff.p;
  if (L.ov) {
    // the launch before last read this index: its k_decode must be through with it
    if (p->ov.e_read[p->ov.flip]) HIPCHK(c, hipStreamWaitEvent(L.is, p->ov.e_read[p->ov.flip], 0));
    else HIPCHK(c, hipEventCreateWithFlags(&p->ov.e_read[p->ov.flip].p, hipEventDisableTiming));
  }
  return MI_RTJ_OK;
}

// ---- stage 2: the speculative index (rtj_spec_kernels.h) ----
// Noisy content defeats the speculation; a plan that sees every packet refused twice in a row goes without it for
// kSpecPauseLaunches launches.  The policy lives on the device (k_spec_policy), so it also works when launches are
// queued faster than they run.
struct SpecGrids {
  dim3 walk, verify, repair;
};
int stage_spec_index(Launch& L, const SpecGrids& g) {
  mi_rtj_plan* p = L.p;
  SpecIndex& s = p->spec;
  const QTab* lut = L.c->d_lut;
  const int mode = p->sw.spec_mode;
  const bool no_policy = mode == 1 || mode == 3 || mode == 4;  // always speculate: short (1), long (3) or very long (4) lead
  L.state = no_policy ? nullptr : s.state.p;
  L.ntodo = s.todo;
  L.todo = s.todo + 1;
  const SpecRunArgs ra = s.run_s > 1u ? SpecRunArgs{s.runs.p, (uint32_t)s.nruns, s.run_s, s.runrec.p, s.rbase.p, s.brow.p}
                                         : SpecRunArgs{nullptr, 0u, 1u, nullptr, nullptr, nullptr};
  STAGE_CHK(L.clk.begin());
  launch_spec_walk(!p->one_block_type, mode, L.state, g.walk, L.is,
                   WalkArgs{p->d_frames, s.chunks, (uint32_t)s.n, L.st, lut, s.rec, s.nrec, s.wstart, s.hand, SpecReset{s.nfix, s.todo, s.flag}, ra});
  STAGE_CHK(L.clk.end(MI_RTJ_K_SPEC_WALK));
  STAGE_CHK(L.clk.begin());
  // first pass; walkers that had not fallen into step are walked again from a known block start; second pass over the
  // packets concerned (both return at once when there is nothing to repair)
  for (int pass = 1; pass <= 2; pass++) {
    if (ra.runs)
      hipLaunchKernelGGL(k_spec_verify<true>, g.verify, dim3(kSpecVerThreads), 0, L.is, p->d_frames, s.base, lut, s.rec, s.nrec, L.blk,
                         s.ok, s.todo + 1, s.todo, L.state, s.wstart, s.hand, s.fix, s.nfix, s.flag, pass, ra);
    else
      hipLaunchKernelGGL(k_spec_verify<false>, g.verify, dim3(kSpecVerThreads), 0, L.is, p->d_frames, s.base, lut, s.rec, s.nrec, L.blk,
                         s.ok, s.todo + 1, s.todo, L.state, s.wstart, s.hand, s.fix, s.nfix, s.flag, pass, ra);
    if (pass == 1)
      hipLaunchKernelGGL(k_spec_repair, g.repair, dim3(64), 0, L.is, p->d_frames, s.chunks, L.st, lut, s.rec, s.nrec, s.wstart,
                         s.hand, s.fix, s.nfix, s.flag, (uint32_t)s.n, L.state, ra.brow);
  }
  STAGE_CHK(L.clk.end(MI_RTJ_K_SPEC_VERIFY));
  if (L.state)
    hipLaunchKernelGGL(k_spec_policy, dim3(1), dim3(256), 0, L.is, (uint32_t)p->n, (uint32_t)s.n, s.todo, s.nfix, L.state, p->sw.serial_min);
  return MI_RTJ_OK;
}

// ---- stage 3: the exact index — the serial walker (MI_RTJ_INDEX=serial), or summarize / resolve / emit over every
// packet or over the speculative index's to-do list ----
struct ExactGrids {
  dim3 walk, walk_todo, summarize, resolve, emit;
};
int stage_exact_index(Launch& L, const ExactGrids& g) {
  mi_rtj_plan* p = L.p;
  const QTab* lut = L.c->d_lut;
  const ChunkIndex& ch = p->chunk;
  if (p->sw.serial_index) {
    STAGE_CHK(L.clk.begin());
    hipLaunchKernelGGL(k_index_walk, g.walk, dim3(64), 0, L.is, p->d_frames, L.st, lut, L.blk);
    return L.clk.end(MI_RTJ_K_EMIT);
  }
  const uint32_t *todo = L.todo, *ntodo = L.ntodo;
  STAGE_CHK(L.clk.begin());
  // A long to-do list (the speculation paused on noisy content, a big launch) goes to the serial walker, one wave
  // per packet: with thousands of packets in flight it indexes faster than the chunk-parallel kernels, whose work
  // grows with the stream's bytes (profiles/r04/noisy_serial_ab.txt: +15 % at 4096 packets of +-64 noise, +28 % at
  // 16384).  k_spec_policy moved the count to the walker's word; the exact kernels then see an empty list.
  if (todo && L.state)
    hipLaunchKernelGGL(k_index_walk_todo, g.walk_todo, dim3(64), 0, L.is, p->d_frames, L.st, lut, L.blk, todo, p->spec.todo + 1 + p->n);
  if (todo) {
    if (p->one_block_type)
      hipLaunchKernelGGL(k_index_summarize_todo<1>, g.summarize, dim3(kSumThreads), 0, L.is, p->d_frames, L.st, lut, ch.summary.p, ch.lentab.p, todo, ntodo);
    else
      hipLaunchKernelGGL(k_index_summarize_todo<2>, g.summarize, dim3(kSumThreads), 0, L.is, p->d_frames, L.st, lut, ch.summary.p, ch.lentab.p, todo, ntodo);
  } else if (p->one_block_type) {
    hipLaunchKernelGGL(k_index_summarize<1>, g.summarize, dim3(kSumThreads), 0, L.is, p->d_frames, L.st, lut, ch.summary.p, ch.lentab.p);
  } else {
    hipLaunchKernelGGL(k_index_summarize<2>, g.summarize, dim3(kSumThreads), 0, L.is, p->d_frames, L.st, lut, ch.summary.p, ch.lentab.p);
  }
  STAGE_CHK(L.clk.end(MI_RTJ_K_SUMMARIZE));
  STAGE_CHK(L.clk.begin());
  hipLaunchKernelGGL(k_index_resolve, g.resolve, dim3(256), 0, L.is, p->d_frames, ch.summary.p, ch.pos.p, ch.mb.p, todo, ntodo);
  STAGE_CHK(L.clk.end(MI_RTJ_K_RESOLVE));
  STAGE_CHK(L.clk.begin());
  if (p->sw.emit_walk)
    hipLaunchKernelGGL(k_index_emit_walk, g.emit, dim3(64), 0, L.is, p->d_frames, L.st, lut, ch.pos.p, ch.mb.p, L.blk);
  else
    hipLaunchKernelGGL(k_index_emit, g.emit, dim3(kEmitThreads), 0, L.is, p->d_frames, ch.lentab.p, ch.pos.p, ch.mb.p, L.blk, todo, ntodo);
  return L.clk.end(MI_RTJ_K_EMIT);
}

// ---- stage 4: from the index kernels' stream to the transform's ----
int launch_hand_over(Launch& L, int what) {
  mi_rtj_plan* p = L.p;
  if (L.is != L.ds) {  // k_decode waits for the index (and, through it, for the packet's copy in)
    if (!p->ov.e_idx) HIPCHK(L.c, hipEventCreateWithFlags(&p->ov.e_idx.p, hipEventDisableTiming));
    HIPCHK(L.c, hipEventRecord(p->ov.e_idx, L.is));
    HIPCHK(L.c, hipStreamWaitEvent(L.ds, p->ov.e_idx, 0));
    L.clk.prev = nullptr;  // (profiling) k_decode's start is not the end of a kernel on another stream
  }
  L.clk.cur = L.ds;
  if (what != kLaunchAll) L.clk.prev = nullptr;  // (profiling) k_decode's start is not the end of the kernel queued before it
  return MI_RTJ_OK;
}

// ---- stage 5: the transform ----
struct Transform {
  const FrameDev* fr;  // the first picture's descriptor
  uint8_t* out;
  dim3 grid, block;    // of the classic form
};

// Batches: what k_decode_split leaves to k_decode_list (DecList) — every part of every group of a launch fits — with its
// counters and the policy's words, made before the first launch that needs them.  A launch that needs a longer list
// waits for the ones queued before it.
int ensure_split_lists(mi_rtj_plan* p, uint64_t need) {
  mi_rtj_ctx* c = p->ctx;
  SplitLists& s = p->split;
  if (s.list.cap < need) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.list.release();
    if (need > 0xFFFFFFFFull) return fail(c, MI_RTJ_ERR_ARG, "plan too large: %llu group parts", (unsigned long long)need);
    STAGE_CHK(s.list.grow(c, need, nullptr));
  }
  if (!s.cnt) {  // two list counters, then the policy's two words (mode, launches left in it)
    STAGE_CHK(s.cnt.grow(c, 4, c->stream, 0, true));
    if (s.h_mode_seen.alloc(1, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer((void**)&s.d_mode_seen, s.h_mode_seen.p, 0) == hipSuccess) {
      *s.h_mode_seen.p = 0xFFFFFFFFu;  // nothing seen yet: both forms are enqueued
    } else {  // (no mapped host memory: both forms are enqueued on every launch, as before)
      (void)hipGetLastError();
      s.h_mode_seen.release();
      s.d_mode_seen = nullptr;
    }
  }
  return MI_RTJ_OK;
}

// batches: luma waves (two parts of their groups in turn) and chroma waves that pool three groups' busy blocks into one
// transform round; what neither covers goes to the list and k_decode_list (rtj_decode_chroma.h)
int stage_transform_split(Launch& L, const Transform& T, dim3 sgrid, dim3 lgrid, uint32_t lw, uint32_t cw, const LaunchExperiments& x,
                          uint64_t need) {
  mi_rtj_plan* p = L.p;
  SplitLists& s = p->split;
  const QTab* lut = L.c->d_lut;
  STAGE_CHK(L.clk.begin());
  uint32_t* const policy = p->sw.split < 0 ? s.cnt + 2 : nullptr;  // (forced split: no policy)
  const bool split_seen = policy && s.h_mode_seen && *(volatile uint32_t*)s.h_mode_seen.p == (uint32_t)kDecModeSplit;
  const DecList list{s.cnt + s.flip, s.list, (uint32_t)s.list.cap};
  // (the device's word decides while the host has not seen the split mode; one kind of wave alone: no policy)
  hipLaunchKernelGGL(k_decode_split, sgrid, T.block, 0, L.ds, T.fr, L.st, lut, L.blk, T.out, lw, cw, list,
                     split_seen || x.split_only ? (const uint32_t*)nullptr : (const uint32_t*)policy, x.xcd_rot);
  // the classic form: runs while the policy says so (returns at once otherwise), and is not enqueued while the host
  // has seen the policy in its split mode (h_mode_seen)
  if (policy && !split_seen)
    hipLaunchKernelGGL((k_decode<true, false>), T.grid, T.block, 0, L.ds, T.fr, L.st, lut, L.blk, T.out, (const uint8_t*)nullptr,
                       (const uint32_t*)policy);
  hipLaunchKernelGGL(k_decode_list, lgrid, T.block, 0, L.ds, T.fr, L.st, lut, L.blk, T.out, list, s.cnt + (s.flip ^ 1), policy,
                     (uint32_t)need, policy ? s.d_mode_seen : nullptr);
  s.flip ^= 1;
  return L.clk.end(MI_RTJ_K_DECODE);
}

// four instantiations: (a wave takes all three parts of its groups | one part) x (unchanged blocks stay | are fetched
// from the previous packet's picture); a launch runs the one that carries nothing else
int stage_transform_classic(Launch& L, const Transform& T, bool all_parts) {
  mi_rtj_plan* p = L.p;
  const QTab* lut = L.c->d_lut;
  const uint32_t* const no_policy = nullptr;
  STAGE_CHK(L.clk.begin());
  if (all_parts) {
    if (p->prev_pic)
      hipLaunchKernelGGL((k_decode<true, true>), T.grid, T.block, 0, L.ds, T.fr, L.st, lut, L.blk, T.out, p->prev_pic, no_policy);
    else
      hipLaunchKernelGGL((k_decode<true, false>), T.grid, T.block, 0, L.ds, T.fr, L.st, lut, L.blk, T.out, (const uint8_t*)nullptr, no_policy);
  } else {
    if (p->prev_pic)
      hipLaunchKernelGGL((k_decode<false, true>), T.grid, T.block, 0, L.ds, T.fr, L.st, lut, L.blk, T.out, p->prev_pic, no_policy);
    else
      hipLaunchKernelGGL((k_decode<false, false>), T.grid, T.block, 0, L.ds, T.fr, L.st, lut, L.blk, T.out, (const uint8_t*)nullptr, no_policy);
  }
  return L.clk.end(MI_RTJ_K_DECODE);
}

// ---- stage 6: phase 2 of a plan with runs: unchanged blocks from the run's earlier pictures, read from this launch's index ----
// (the three kernels of the plan's format; one set of books: run_ev, and launch_close / launch_fmt note runs_ran)
template <int Fmt>
void queue_runs(Launch& L, const RunGrids& g, uint8_t* out) {
  mi_rtj_plan* p = L.p;
  const Runs& r = p->runs;
  hipLaunchKernelGGL(k_runs_mask<Fmt>, g.mask, dim3(kRunScanThreads), 0, L.ds, p->d_frames, r.d_chunks, r.chunks, (const uint32_t*)L.blk, r.d_mask);
  hipLaunchKernelGGL(k_runs_carry<Fmt>, g.carry, dim3(kRunScanThreads), 0, L.ds, r.d_runs, r.list, r.d_chunks, r.d_mask, r.d_carry, r.d_copied);
  hipLaunchKernelGGL(k_runs_copy<Fmt>, g.copy, dim3(g.copy_threads), 0, L.ds, p->d_frames, r.d_chunks, g.items, r.d_mask, r.d_carry, out, r.d_copied);
}

int stage_runs(Launch& L, bool runs, const RunGrids& g, uint8_t* out) {
  mi_rtj_plan* p = L.p;
  if (p->profile) {
    Timed rt;
    rt.a = L.clk.prev;
    if (runs) STAGE_CHK(timing_event(p, &rt.b));
    p->run_ev.push_back(rt);
  }
  if (!runs) return MI_RTJ_OK;
  switch (p->fmt) {
    case MI_RTJ_FMT_YUV422: queue_runs<kFmtYUV422>(L, g, out); break;
    case MI_RTJ_FMT_GREY: queue_runs<kFmtGrey>(L, g, out); break;
    default: queue_runs<kFmtYUV420>(L, g, out); break;
  }
  if (p->profile) HIPCHK(L.c, hipEventRecord(p->run_ev.back().b, L.ds));
  return MI_RTJ_OK;
}

// ---- stage 7: the books ----
int launch_close(Launch& L, int what, bool runs) {
  mi_rtj_plan* p = L.p;
  if (what == kLaunchAll) p->runs_ran = runs;
  HIPCHK(L.c, hipGetLastError());
  if (L.ov) {
    HIPCHK(L.c, hipEventRecord(p->ov.e_read[p->ov.flip], L.ds));
    p->ov.last = p->ov.flip;
    p->ov.flip ^= 1;
  } else {
    p->ov.last = 0;
  }
  if (what == kLaunchAll) p->ov.last_overlapped = L.ov && L.is != L.ds;
  p->launches++;
  return MI_RTJ_OK;
}

}  // namespace
