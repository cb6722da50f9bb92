// rtj_host_pipe.h — pipelined session (mi_rtj_pipe_*): the decoder a frame-owning plugin instance reads ahead with
// (lib/video.c:420-441 nocopy source, lib/video_v4l2_m2m.c:43-131 as the in-tree precedent of a decoder with packets in
// flight).  Included by mi_rtjpeg.hip behind the plan's state and plan_launch().
#pragma once

// One packet in flight of a pipelined session: its own pinned staging, device packet, device picture, pinned host
// picture and one-frame plan, so that the copy in of packet i+1, the kernels of packet i and the copy out of picture
// i-1 run side by side on three streams.
struct PipeSlot {
  mi_rtj_plan* plan = nullptr;
  FlagPinnedBuf<uint8_t> h_stage;  // FrameDev (64 bytes), then the packet
  DevBuf<uint8_t> d_stage;     // (its capacity is the staging's)
  DevBuf<uint8_t> own_d_pic;   // the slot's own pictures (sessions without copy groups) ...
  FlagPinnedBuf<uint8_t> own_h_pic;
  uint8_t* d_pic = nullptr;    // ... and the ones in use: this packet's picture on the device (starts as a copy of its
  uint8_t* h_pic = nullptr;    // predecessor's) and the pinned host picture handed to the caller
  size_t pic_cap = 0;
  bool owns_pic = true;        // false: d_pic / h_pic point into the session's group buffers (copies out in groups)
  int out_state = 0;           // 0 nothing to copy, 1 decoded and waiting for its group's copy out, 2 copy out queued
  hipEvent_t out_ev = nullptr; // the event that says this picture is in host memory (e_out of the slot that closed the copy; borrowed)
  Event e_in, e_dec, e_out;    // (the slots go before the session's streams: mi_rtj_pipe)
  uint64_t tag = 0;
  int w = 0, h = 0;
  FrameDev fd;                      // (index groups) the packet's descriptor, bases filled in when its group is queued
  int staged = 0;                   // (index groups) 1: copied in, kernels not queued yet
  // hand-over to the session's worker thread (the HIP calls of a packet are made there)
  size_t len = 0;                   // packet bytes in h_stage
  const uint8_t* prev = nullptr;    // predecessor's device picture (or none)
  int issued = 0;                   // 1 once the worker has queued everything up to the copy out (guarded by mu)
  int rc = 0;                       // what queuing it returned
  std::string err;

  PipeSlot() = default;
  // out of line and hidden: the loop that moves the slots (slot.resize(), once a session) then stays inside the vector's
  // own function, and the library exports the symbols it did while the events were raw handles
  __attribute__((noinline, visibility("hidden"))) PipeSlot(PipeSlot&&) noexcept;
};
inline PipeSlot::PipeSlot(PipeSlot&&) noexcept = default;

struct mi_rtj_pipe {
  mi_rtj_ctx* ctx = nullptr;
  int depth = 0;
  int max_w = 0, max_h = 0;   // the stream's coded size: packets that announce more are refused
  // Members are destroyed last to first: the streams are declared in front of the slots and the buffers, whose events
  // were recorded on them.
  // kernels run on the instance's stream; packets come in on s_in; pictures leave on s_out[slot & 1]: with one stream a
  // session has one picture-sized copy out in flight at a time, and the link gives such a copy (3.1 MB at 1080p) 38 GB/s
  // where two side by side, or larger ones, get past 50 (profiles/r02/pcie_probe.json); MI_RTJ_OUT_STREAMS=1 is the A/B
  Stream s_in, s_out[2];
  Stream s_idx;               // MI_RTJ_IDX_STREAM=1 (A/B, slower): index kernels of the packets on a stream of their own
  std::vector<PipeSlot> slot;
  int head = 0, count = 0;    // oldest packet in flight, packets in flight
  int lent = -1;              // slot whose host picture the caller is looking at (until the next mi_rtj_pipe_next)
  const uint8_t* prev_pic = nullptr;  // device picture of the packet submitted last (what 0xFF blocks keep)
  size_t prev_bytes = 0;
  // The session's environment switches (rtj_host_switches.h).  stats: where the submitting thread's time goes is printed
  // to stderr when the session ends; threaded: HIP calls on the worker thread (A/B; off by default)
  PipeSwitches sw;
  // Pictures leave in groups: the slots of a group lie side by side on the device and in pinned host memory, and one
  // copy takes all of them once the group's last packet is decoded (or as many as are decoded when the caller asks for
  // one earlier).  The link moves a 1080p picture (3.1 MB) at 38 GB/s and 6-12 MB at 47-55 (profiles/r02/pcie_probe.json),
  // and two copy streams do NOT overlap two small copies (profiles/r03/e2e_what_bounds_a_session.txt).
  // MI_RTJ_OUT_GROUP = 1 / 2 / 4; sessions without a fixed coded size copy picture by picture.
  int group = 1;
  size_t grp_fsz = 0;                    // bytes of one picture in a group buffer
  std::vector<DevBuf<uint8_t>> d_grp;    // [depth / group]
  std::vector<FlagPinnedBuf<uint8_t>> h_grp;
  // The INDEX of the packets is built in groups as well (MI_RTJ_IDX_GROUP = 1 / 2 / 4, default: the copy group): the
  // exact index of ONE 1080p packet is three launches that each run one round of workgroups or one serial chain
  // (k_index_summarize 19 us, k_index_resolve 21, k_index_emit 13, tools/one_packet_kernels.py) and take as long for
  // two or four packets side by side.  A packet is copied in at once and waits ("staged") until its group is complete
  // or the caller asks for its picture; then one index launch covers the group and k_decode follows packet by packet
  // (a packet's unchanged blocks come from its predecessor's picture).  One plan per group of slots; the descriptors
  // of all slots live in one array (pinned + device) so that a group's are contiguous.
  int igroup = 1;
  int nstaged = 0;                     // slots staged and not yet queued: the last `nstaged` submitted
  std::vector<mi_rtj_plan*> gplan;     // [depth / igroup]
  FlagPinnedBuf<FrameDev> h_desc;      // [depth]
  DevBuf<FrameDev> d_desc;             // [depth]
  uint64_t submitted = 0, returned = 0;
  // MI_RTJ_PIPE_STATS=1 (seconds): [0] copying packets into pinned staging, [1] runtime calls that queue work, [2] waiting
  // for a picture's copy out; t_d2h_call: inside hipMemcpyAsync of the copy out (part of t_issue)
  double t_stage = 0, t_issue = 0, t_wait = 0, t_d2h_call = 0;
  // The thread that submits is what bounds a session (about 50 us of runtime calls per packet next to the 30 us it
  // takes to copy a 1080p packet into pinned staging), so the two halves run on two threads: the caller copies, a
  // worker owned by the session makes the HIP calls, in submission order.
  std::thread worker;
  std::mutex mu;
  std::condition_variable cv_work, cv_done;
  std::vector<int> jobs;      // ring of slot numbers waiting for the worker
  size_t job_head = 0, job_count = 0;
  bool stop = false;
};

namespace {
inline double host_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// how the pinned host pictures are allocated (MI_RTJ_HOST_FLAGS, experiments: 1 non-coherent, 2 coherent, 4 write-combined)
unsigned pic_host_flags() {
  const char* f = exp_env("MI_RTJ_HOST_FLAGS");
  const int v = f ? atoi(f) : 0;
  unsigned fl = hipHostMallocDefault;
  if (v & 1) fl |= hipHostMallocNonCoherent;
  if (v & 2) fl |= hipHostMallocCoherent;
  if (v & 4) fl |= hipHostMallocWriteCombined;
  return fl;
}

// queue the copy out of slot `last` together with the decoded, not yet copied slots of its group right before it
int pipe_copy_out(mi_rtj_pipe* q, int last) {
  mi_rtj_ctx* c = q->ctx;
  int first = last;
  while (first % q->group != 0 && q->slot[first - 1].out_state == 1 && q->slot[first - 1].w == q->slot[last].w &&
         q->slot[first - 1].h == q->slot[last].h)
    first--;
  PipeSlot& a = q->slot[first];
  PipeSlot& z = q->slot[last];
  const size_t fsz = (size_t)z.w * z.h * 3 / 2;
  const size_t bytes = (size_t)(z.d_pic - a.d_pic) + fsz;  // one slot: fsz; a group: its members lie side by side
  hipStream_t so = q->s_out[(last / q->group) % q->sw.out_streams];
  // "decoded" is recorded here, once per copy, not behind every packet's k_decode: the kernels of the group's members
  // were queued before this point on the same stream (whatever else was queued behind them merely makes the copy wait
  // a little longer: that only happens when the caller asks for a picture of an incomplete group)
  HIPCHK(c, hipEventRecord(z.e_dec, c->stream));
  HIPCHK(c, hipStreamWaitEvent(so, z.e_dec, 0));
  if (q->sw.exp_skip & 1) {
  } else if (q->sw.out_kernel) {
    hipLaunchKernelGGL(k_copy16, dim3(q->sw.out_kernel), dim3(256), 0, so, (const uint4*)a.d_pic, (uint4*)a.h_pic, bytes / 16);
  } else {
    const double t0 = q->sw.stats ? host_now() : 0.0;
    HIPCHK(c, hipMemcpyAsync(a.h_pic, a.d_pic, bytes, hipMemcpyDeviceToHost, so));
    if (q->sw.stats) q->t_d2h_call += host_now() - t0;
  }
  HIPCHK(c, hipEventRecord(z.e_out, so));
  for (int i = first; i <= last; i++) {
    q->slot[i].out_state = 2;
    q->slot[i].out_ev = z.e_out;
  }
  return MI_RTJ_OK;
}

// everything of one packet that goes to the device: copy in, kernels, copy out (called on the worker thread, or on
// the caller's when the session runs without one)
int pipe_issue(mi_rtj_pipe* q, PipeSlot& sl) {
  mi_rtj_ctx* c = q->ctx;
  mi_rtj_plan* p = sl.plan;
  // (the copy in has a stream of its own: queued between the kernels of successive packets the session ran at
  // 6-10 K pictures per second instead of 12 K, and the deeper the pipeline the slower — profiles/r02/e2e_*.txt)
  if (!(q->sw.exp_skip & 4))
    HIPCHK(c, hipMemcpyAsync(sl.d_stage, sl.h_stage, sizeof(FrameDev) + sl.len, hipMemcpyHostToDevice, q->s_in));
  HIPCHK(c, hipEventRecord(sl.e_in, q->s_in));
  HIPCHK(c, hipStreamWaitEvent(p->idx_stream ? p->idx_stream : c->stream, sl.e_in, 0));
  // kernels, in submission order on the instance's stream.  Unchanged (0xFF) blocks: k_decode fetches them from the
  // predecessor's picture (a packet of another size has no predecessor in that sense: its unchanged blocks keep what
  // the slot's buffer holds, zeros at first)
  p->prev_pic = sl.prev;
  const int rc = (q->sw.exp_skip & 2) ? MI_RTJ_OK : plan_launch(p, sl.d_stage, sl.d_pic);
  if (rc != MI_RTJ_OK) return rc;
  // copy out: queued now if this packet closes its group, else when the group's last packet is decoded or the caller
  // asks for one of its pictures, whichever comes first
  sl.out_state = 1;
  const int idx = (int)(&sl - q->slot.data());
  if (idx % q->group == q->group - 1) return pipe_copy_out(q, idx);
  return MI_RTJ_OK;
}

// ---- index groups: copy in now, kernels when the group is complete ----
int pipe_stage(mi_rtj_pipe* q, PipeSlot& sl) {
  mi_rtj_ctx* c = q->ctx;
  if (!(q->sw.exp_skip & 4))
    HIPCHK(c, hipMemcpyAsync(sl.d_stage, sl.h_stage, sizeof(FrameDev) + sl.len, hipMemcpyHostToDevice, q->s_in));
  sl.staged = 1;
  sl.out_state = 0;
  q->nstaged++;
  return MI_RTJ_OK;
}

// queue the kernels of the `count` staged slots first .. first + count - 1 (one aligned group or a part of one)
int pipe_issue_group(mi_rtj_pipe* q, int first, int count) {
  mi_rtj_ctx* c = q->ctx;
  mi_rtj_plan* p = q->gplan[first / q->igroup];
  p->n = count;
  p->h_frames.resize((size_t)count);
  uint64_t nidx = 0;
  p->max_groups = 0;
  p->n_blocks = 0;
  for (int j = 0; j < count; j++) {
    FrameDev& f = q->slot[first + j].fd;
    f.blk_base = (uint32_t)nidx;
    nidx += frame_index_entries(f, p->fmt);
    p->n_blocks += frame_blocks(f, p->fmt);
    p->max_groups = std::max(p->max_groups, frame_groups(f, p->fmt));
    p->h_frames[(size_t)j] = f;
  }
  int rc = plan_fit_index(p, nidx, nidx / (uint64_t)count * (uint64_t)q->igroup);  // room for a whole group of such pictures
  if (rc != MI_RTJ_OK) return rc;
  // chunk bases of the group's packets; allocates only when the group outgrows its buffers
  if ((rc = plan_alloc_chunks(p)) != MI_RTJ_OK) return rc;
  // the descriptors follow the packets on the copy-in stream; the kernels wait for both
  for (int j = 0; j < count; j++) q->h_desc[first + j] = p->h_frames[(size_t)j];
  HIPCHK(c, hipMemcpyAsync(q->d_desc + first, q->h_desc + first, sizeof(FrameDev) * (size_t)count, hipMemcpyHostToDevice, q->s_in));
  PipeSlot& lastsl = q->slot[first + count - 1];
  HIPCHK(c, hipEventRecord(lastsl.e_in, q->s_in));
  HIPCHK(c, hipStreamWaitEvent(c->stream, lastsl.e_in, 0));
  p->d_frames = q->d_desc + first;
  // (data_off of these descriptors is the packet's device ADDRESS: the kernels add it to a null stream base)
  if (!(q->sw.exp_skip & 2)) {
    p->prev_pic = nullptr;
    if ((rc = plan_launch(p, nullptr, nullptr, kLaunchIndex)) != MI_RTJ_OK) return rc;
  }
  for (int j = 0; j < count; j++) {
    PipeSlot& sl = q->slot[first + j];
    if (!(q->sw.exp_skip & 2)) {
      p->prev_pic = sl.prev;
      if ((rc = plan_launch(p, nullptr, sl.d_pic, kLaunchDecode, (uint32_t)j, 1)) != MI_RTJ_OK) return rc;
    }
    sl.staged = 0;
    sl.out_state = 1;
    q->nstaged--;
    if ((first + j) % q->group == q->group - 1 && (rc = pipe_copy_out(q, first + j)) != MI_RTJ_OK) return rc;
  }
  return MI_RTJ_OK;
}

// the staged slots are the last q->nstaged submitted ones; queue their kernels
int pipe_issue_staged(mi_rtj_pipe* q) {
  if (q->nstaged <= 0) return MI_RTJ_OK;
  const int count = q->nstaged;
  const int last = (q->head + q->count - 1 + q->depth) % q->depth;
  const int first = last - (count - 1);  // a group never wraps: the depth is a multiple of the group size
  const int rc = pipe_issue_group(q, first, count);
  if (rc != MI_RTJ_OK) {  // what could not be queued yields no pictures
    for (int j = 0; j < count; j++) {
      PipeSlot& sl = q->slot[first + j];
      if (sl.staged) {
        sl.staged = 0;
        sl.rc = rc;
        sl.err = q->ctx->err;
      }
    }
    q->nstaged = 0;
  }
  return rc;
}

void pipe_worker(mi_rtj_pipe* q) {
  (void)hipSetDevice(q->ctx->device);
  for (;;) {
    int idx;
    {
      std::unique_lock<std::mutex> lk(q->mu);
      q->cv_work.wait(lk, [&] { return q->stop || q->job_count > 0; });
      if (q->job_count == 0) return;  // stop, and nothing left to queue
      idx = q->jobs[q->job_head];
    }
    PipeSlot& sl = q->slot[idx];
    const int rc = pipe_issue(q, sl);
    {
      std::lock_guard<std::mutex> lk(q->mu);
      sl.rc = rc;
      if (rc != MI_RTJ_OK) sl.err = q->ctx->err;
      sl.issued = 1;
      q->job_head = (q->job_head + 1) % q->jobs.size();
      q->job_count--;
    }
    q->cv_done.notify_all();
  }
}

// wait until the worker has nothing left to queue (allocation changes, flush, destroy)
void pipe_drain_jobs(mi_rtj_pipe* q) {
  if (!q->sw.threaded) return;
  std::unique_lock<std::mutex> lk(q->mu);
  q->cv_done.wait(lk, [&] { return q->job_count == 0; });
}
}  // namespace

extern "C" {

mi_rtj_pipe* mi_rtj_pipe_create(mi_rtj_ctx* c, int depth, int max_w, int max_h) {
  if (!c || depth < 2 || depth > 64 || max_w < 0 || max_h < 0) {
    fail(c, MI_RTJ_ERR_ARG, "mi_rtj_pipe_create: bad argument (depth 2..64)");
    return nullptr;
  }
  if (c->fmt != MI_RTJ_FMT_YUV420) {
    fail(c, MI_RTJ_ERR_ARG, "mi_rtj_pipe_create: sessions decode 4:2:0 streams only; this instance's format is %s",
         kFormats[c->fmt].abi_name);
    return nullptr;
  }
  if (hipSetDevice(c->device) != hipSuccess) {
    fail(c, MI_RTJ_ERR_HIP, "mi_rtj_pipe_create: hipSetDevice failed");
    return nullptr;
  }
  c->fmt_fixed = true;
  mi_rtj_pipe* q = new mi_rtj_pipe();
  q->ctx = c;
  q->max_w = max_w;
  q->max_h = max_h;
  q->sw = pipe_switches_from_env();
  {
    // fours from twelve packets in flight on (three groups: one being copied, one queued behind it, one being filled):
    // 16.0-16.2 K pictures per second at 1080p against 15.0 K in pairs, 4.36 K at 4K against 4.26 K (the link gives
    // 4.39 K); with two groups of four the copy engine idles while the caller refills one (9.9 K)
    const int g = q->sw.out_group_set ? q->sw.out_group : depth >= 12 ? 4 : 2;
    // (groups need every picture to have the session's size, and the caller's thread to be the one that queues copies)
    const bool may_group = max_w > 0 && max_h > 0 && !q->sw.threaded;
    q->group = may_group && (g == 2 || g == 4) ? g : 1;
    // the index is built in groups too, by default the same ones (needs the same things: one coded size, the
    // caller's thread queuing the work); MI_RTJ_IDX_GROUP = 1 is the packet-by-packet index of rounds 2 and 3
    const int igv = q->sw.idx_group_set ? q->sw.idx_group : q->group;
    q->igroup = may_group && (igv == 2 || igv == 4) ? igv : 1;
    const int unit = std::max(q->group, q->igroup);  // (1, 2 or 4 each: the larger is a multiple of the other)
    depth = (depth + unit - 1) / unit * unit;
    if (q->group > 1) q->grp_fsz = (size_t)max_w * max_h * 3 / 2;
  }
  q->depth = depth;
  q->slot.resize(depth);
  // The runtime multiplexes the streams of a process onto a few hardware queues PER PRIORITY (four by default,
  // GPU_MAX_HW_QUEUES): with every stream at the default priority two sessions' eight streams shared four queues and one
  // session's copy in waited behind the other's copy out (two sessions then aggregated LESS than one).
  // The copy streams of a session are therefore created at the two other priorities the device offers — packets in at
  // the highest, pictures out at the lowest — which puts them into queue pools of their own: kernels, copies in and
  // copies out of several sessions no longer meet in one queue, and the application need not set anything.  (For copies
  // the priority itself changes nothing: they run on the copy engines.)  MI_RTJ_STREAM_PRIO=0: all default (A/B).
  int prio_lo = 0, prio_hi = 0;  // numerically: lowest priority = largest value
  if (!q->sw.stream_prio || hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_lo = prio_hi = 0;
  auto make_stream = [&](hipStream_t* st, int prio) {
    return (prio_lo != prio_hi ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio)
                               : hipStreamCreateWithFlags(st, hipStreamNonBlocking)) == hipSuccess;
  };
  bool ok = make_stream(&q->s_in.p, prio_hi);
  // off unless asked for: with the index on a stream of its own a 1080p session ran at 6,600 pictures per second
  // instead of 12,000 (profiles/r03/e2e_ab.txt) — every packet then crosses streams twice more, and the runtime's
  // cross-stream waits cost more than the overlap of one packet's index with its predecessor's transform gives
  if (q->sw.idx_stream) ok = ok && hipStreamCreateWithFlags(&q->s_idx.p, hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; i < q->sw.out_streams; i++) ok = ok && make_stream(&q->s_out[i].p, prio_lo);
  for (auto& sl : q->slot) {
    sl.plan = plan_new(c, 1, kPlanSessionSlot);
    sl.plan->idx_stream = q->s_idx;
    ok = ok && hipEventCreateWithFlags(&sl.e_in.p, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&sl.e_dec.p, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&sl.e_out.p, hipEventDisableTiming) == hipSuccess;
  }
  if (ok && q->igroup > 1) {  // one plan per index group, the descriptors of all slots in one array
    ok = q->h_desc.alloc((uint64_t)depth) == hipSuccess && q->d_desc.grow(c, (uint64_t)depth, c->stream) == MI_RTJ_OK;
    q->gplan.assign((size_t)(depth / q->igroup), nullptr);
    for (auto& gp : q->gplan) gp = plan_new(c, q->igroup, kPlanSessionGroup);
  }
  if (ok && q->group > 1) {  // the group buffers: `group` pictures side by side, on the device and in pinned host memory
    const int ng = depth / q->group;
    q->d_grp.resize(ng);
    q->h_grp.resize(ng);
    const size_t gb = q->grp_fsz * (size_t)q->group;
    for (int g = 0; g < ng && ok; g++) {
      ok = q->d_grp[g].grow(c, gb, c->stream, kAllocPad, true) == MI_RTJ_OK && q->h_grp[g].alloc(gb, pic_host_flags()) == hipSuccess;
      for (int j = 0; j < q->group && ok; j++) {
        PipeSlot& sl = q->slot[g * q->group + j];
        sl.d_pic = q->d_grp[g] + (size_t)j * q->grp_fsz;
        sl.h_pic = q->h_grp[g] + (size_t)j * q->grp_fsz;
        sl.pic_cap = q->grp_fsz;
        sl.owns_pic = false;
      }
    }
  }
  if (!ok) {
    fail(c, MI_RTJ_ERR_HIP, "mi_rtj_pipe_create: cannot create streams / events / picture buffers");
    mi_rtj_pipe_destroy(q);
    return nullptr;
  }
  // MI_RTJ_PIPE_THREAD=1: the HIP calls of a packet are made by a worker thread of the session instead of the
  // caller's.  It frees the caller (which then only copies the packet into staging) but buys no throughput where it
  // was hoped to: 12,020 against 12,070 pictures per second at 1080p (the copy out bounds the session there, see
  // DESIGN.md), 20,260 against 18,870 at 320x240 (profiles/r02/e2e_worker_thread.txt).  Off by default.
  q->jobs.assign((size_t)depth, 0);
  if (q->sw.threaded) q->worker = std::thread(pipe_worker, q);
  return q;
}

void mi_rtj_pipe_destroy(mi_rtj_pipe* q) {
  if (!q) return;
  mi_rtj_ctx* c = q->ctx;
  if (q->sw.stats && q->returned)
    fprintf(stderr, "{\"pipe_stats\": {\"pictures\": %llu, \"us_per_picture\": {\"staging_memcpy\": %.1f, \"queueing_calls\": %.1f, \"of_which_the_d2h_memcpy_call\": %.1f, \"waiting_for_copy_out\": %.1f}}}\n",
            (unsigned long long)q->returned, 1e6 * q->t_stage / q->returned, 1e6 * q->t_issue / q->returned, 1e6 * q->t_d2h_call / q->returned, 1e6 * q->t_wait / q->returned);
  (void)hipSetDevice(c->device);
  if (q->worker.joinable()) {
    {
      std::lock_guard<std::mutex> lk(q->mu);
      q->stop = true;
    }
    q->cv_work.notify_all();
    q->worker.join();  // it queues what it still holds, then leaves
  }
  if (q->s_in) (void)hipStreamSynchronize(q->s_in);
  if (q->s_idx) (void)hipStreamSynchronize(q->s_idx);
  (void)hipStreamSynchronize(c->stream);
  for (hipStream_t so : q->s_out)
    if (so) (void)hipStreamSynchronize(so);
  for (auto& sl : q->slot) mi_rtj_plan_destroy(sl.plan);  // (a plan frees what it owns: its descriptors are the slot's staging)
  for (mi_rtj_plan* gp : q->gplan) mi_rtj_plan_destroy(gp);
  if (q->s_idx) (void)hipStreamSynchronize(q->s_idx);
  delete q;  // (the slots' events, staging, pictures, group buffers and descriptors, then the streams)
}

int mi_rtj_pipe_room(const mi_rtj_pipe* q) {
  if (!q) return 0;
  return q->depth - q->count - (q->lent >= 0 ? 1 : 0);
}

int mi_rtj_pipe_pending(const mi_rtj_pipe* q) { return q ? q->count : 0; }

int mi_rtj_pipe_submit(mi_rtj_pipe* q, const uint8_t* pkt, size_t len, uint64_t tag) {
  if (!q || !pkt) return fail(q ? q->ctx : nullptr, MI_RTJ_ERR_ARG, "mi_rtj_pipe_submit: NULL argument");
  mi_rtj_ctx* c = q->ctx;
  const bool stats = q->sw.stats;
  // (an error message is written into the instance, which the worker thread of a threaded session writes too: the
  // worker is idle before any of the refusals below speaks — ADVICE r2)
  if (len < MI_RTJ_HEADER_SIZE || mi_rtj_pipe_room(q) <= 0) pipe_drain_jobs(q);
  if (len < MI_RTJ_HEADER_SIZE) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_pipe_submit: packet shorter than its %d-byte header", MI_RTJ_HEADER_SIZE);
  if (mi_rtj_pipe_room(q) <= 0) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_pipe_submit: %d packets in flight already (take a picture first)", q->count);
  HIPCHK(c, hipSetDevice(c->device));
  const int hw = pkt[6] | (pkt[7] << 8), hh = pkt[8] | (pkt[9] << 8);
  // the header against the stream's size BEFORE anything is allocated for it (a 65520 x 65520 header would ask for
  // gigabytes; the reference's frame has the container's size whatever the packet says, lib/video_rtjpeg.c:50-54)
  if (q->max_w && q->max_h && (hw != q->max_w || hh != q->max_h)) {
    pipe_drain_jobs(q);
    return fail(c, MI_RTJ_ERR_GEOMETRY, "packet header %dx%d does not match the stream's coded size %dx%d", hw, hh, q->max_w, q->max_h);
  }
  // the slots form a ring: the lent one (if any) sits just before head, then head .. head+count-1, then the free ones
  const int idx = (q->head + q->count) % q->depth;
  PipeSlot& sl = q->slot[idx];
  mi_rtj_plan* p = sl.plan;
  // (fill_frame and everything below may write the instance's error string and allocate: the worker must be idle
  // whenever that can happen, i.e. on an error or when a buffer has to grow — not in the steady state)
  FrameDev f;
  {
    const bool geometry_ok = hw > 0 && hh > 0 && !(hw & 15) && !(hh & 15);
    const size_t fsz0 = geometry_ok ? (size_t)hw * hh * 3 / 2 : 0;
    const uint64_t nidx0 = geometry_ok ? ((((uint64_t)(hw / 16) * (hh / 16)) * 6 + 1) + 63) & ~63ull : 0;
    const uint32_t nchunks0 = (uint32_t)((len - MI_RTJ_HEADER_SIZE + kChunk - 1) / kChunk) + 1u;
    const bool grows = !geometry_ok || fsz0 > sl.pic_cap || sizeof(FrameDev) + len + kAllocPad > sl.d_stage.cap ||
                       nidx0 > p->blkoff.cap || nchunks0 > p->chunk.chunks() || (uint64_t)nchunks0 + 1 > p->chunk.entries();
    if (grows) pipe_drain_jobs(q);
  }
  int rc = fill_frame(c, pkt, 0, (uint32_t)len, 0, 0, &f);
  if (rc != MI_RTJ_OK) return rc;
  p->h_frames[0] = f;
  const size_t fsz = (size_t)f.w * f.h * 3 / 2;
  if (fsz > sl.pic_cap && !sl.owns_pic)  // cannot happen: grouped sessions refuse packets of another size above
    return fail(c, MI_RTJ_ERR_GEOMETRY, "mi_rtj_pipe_submit: picture larger than the session's");
  if (fsz > sl.pic_cap) {
    sl.pic_cap = 0;
    sl.d_pic = sl.h_pic = nullptr;
    if ((rc = sl.own_d_pic.grow(c, fsz, c->stream, kAllocPad, true)) != MI_RTJ_OK) return rc;
    HIPCHK(c, sl.own_h_pic.alloc(fsz, pic_host_flags()));
    sl.d_pic = sl.own_d_pic;
    sl.h_pic = sl.own_h_pic;
    sl.pic_cap = fsz;
  }
  const size_t need = sizeof(FrameDev) + len + kAllocPad;
  if (need > sl.d_stage.cap) {
    HIPCHK(c, sl.h_stage.alloc(need * 2));
    if ((rc = sl.d_stage.grow(c, need * 2, c->stream)) != MI_RTJ_OK) return rc;
  }
  const bool grouped = q->igroup > 1;  // the index of this packet is built with its group's (pipe_issue_group)
  if (!grouped) {
    if ((rc = plan_fit_index(p, frame_index_entries(f, p->fmt), 0)) != MI_RTJ_OK) return rc;
    p->n_blocks = frame_blocks(f, p->fmt);
    p->max_groups = frame_groups(f, p->fmt);
    if ((rc = plan_alloc_chunks(p)) != MI_RTJ_OK) return rc;  // sets the chunk bases in the descriptor; allocates only when it grows
  }
  // descriptor and packet travel together: one copy in, on its own stream
  FrameDev& fd = p->h_frames[0];  // plan_alloc_chunks has set its chunk bases
  fd.data_off = sizeof(FrameDev) + MI_RTJ_HEADER_SIZE;
  if (grouped) {
    // the kernels of a group get a null stream base: data_off is the device address of the packet's first data byte
    // (the packets of a group lie in their slots' own buffers); block and chunk bases are set when the group is queued
    fd.data_off = (uint64_t)(uintptr_t)sl.d_stage.p + sizeof(FrameDev) + MI_RTJ_HEADER_SIZE;
    sl.fd = fd;
  }
  const double ts0 = stats ? host_now() : 0.0;
  memcpy(sl.h_stage, &fd, sizeof(FrameDev));
  memcpy(sl.h_stage + sizeof(FrameDev), pkt, len);
  if (stats) q->t_stage += host_now() - ts0;
  p->d_frames = (const FrameDev*)sl.d_stage.p;
  sl.len = len;
  sl.tag = tag;
  sl.w = (int)fd.w;
  sl.h = (int)fd.h;
  const uint8_t* const was_prev = q->prev_pic;
  const size_t was_bytes = q->prev_bytes;
  sl.prev = q->prev_pic && q->prev_bytes == fsz && q->prev_pic != sl.d_pic ? q->prev_pic : nullptr;
  q->prev_pic = sl.d_pic;
  q->prev_bytes = fsz;
  q->count++;
  q->submitted++;
  if (!q->sw.threaded) {
    const double ti0 = stats ? host_now() : 0.0;
    bool group_failed = false;
    if (grouped) {
      sl.rc = pipe_stage(q, sl);
      // the group's last slot: queue the kernels of the whole group.  Should THAT fail, the group's packets are in all
      // the same, this one included: their slots carry the error and yield no pictures, mi_rtj_pipe_next reports it once
      // per packet, and submit returns OK — one behaviour for all members of the group (the last member used
      // to be taken out again and reported twice while its siblings stayed in flight)
      if (sl.rc == MI_RTJ_OK && idx % q->igroup == q->igroup - 1) group_failed = pipe_issue_staged(q) != MI_RTJ_OK;
    } else {
      sl.rc = pipe_issue(q, sl);
    }
    if (stats) q->t_issue += host_now() - ti0;
    sl.issued = 1;
    if (group_failed) return MI_RTJ_OK;
    if (sl.rc != MI_RTJ_OK) {  // this packet's own copy in (or, ungrouped, its kernels) could not be queued: undo — it never
                               // went in, its predecessor is still the last picture
      q->count--;
      q->submitted--;
      q->prev_pic = was_prev;
      q->prev_bytes = was_bytes;
      return sl.rc;
    }
    return MI_RTJ_OK;
  }
  {
    std::lock_guard<std::mutex> lk(q->mu);
    sl.issued = 0;
    sl.rc = MI_RTJ_OK;
    q->jobs[(q->job_head + q->job_count) % q->jobs.size()] = idx;
    q->job_count++;
  }
  q->cv_work.notify_one();
  return MI_RTJ_OK;
}

int mi_rtj_pipe_next(mi_rtj_pipe* q, const uint8_t* planes[3], int strides[3], int* w, int* h, uint64_t* tag) {
  if (!q) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = q->ctx;
  const bool stats = q->sw.stats;
  q->lent = -1;  // the picture handed out before is the caller's no longer
  if (q->count == 0) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_pipe_next: nothing in flight");
  HIPCHK(c, hipSetDevice(c->device));
  PipeSlot& sl = q->slot[q->head];
  if (q->sw.threaded) {
    std::unique_lock<std::mutex> lk(q->mu);
    q->cv_done.wait(lk, [&] { return sl.issued != 0; });
  }
  if (sl.staged) {  // its index group is not complete: the kernels of what is staged are queued now
    const double ti0 = stats ? host_now() : 0.0;
    (void)pipe_issue_staged(q);  // (a failure is in the slots' rc)
    if (stats) q->t_issue += host_now() - ti0;
  }
  if (sl.rc != MI_RTJ_OK) {  // queuing this packet failed (on the worker, or with its group): it yields no picture
    const int rc = sl.rc;
    if (!sl.err.empty()) c->err = sl.err;
    q->head = (q->head + 1) % q->depth;
    q->count--;
    return rc;
  }
  if (sl.out_state == 1) {  // its group is not complete yet: the copy goes out now, with what is decoded behind it
    int last = q->head;
    while ((last + 1) % q->group != 0 && last + 1 < q->depth && q->slot[last + 1].out_state == 1) last++;
    const int rc = pipe_copy_out(q, last);
    if (rc != MI_RTJ_OK) return rc;
  }
  {
    const double tw0 = stats ? host_now() : 0.0;
    hipEvent_t const ev = sl.out_ev ? sl.out_ev : sl.e_out;
    if (q->sw.wait_mode == 1) {  // MI_RTJ_WAIT=query (A/B): poll instead of blocking inside the runtime
      hipError_t e;
      while ((e = hipEventQuery(ev)) == hipErrorNotReady) std::this_thread::yield();
      HIPCHK(c, e);
    } else {
      HIPCHK(c, hipEventSynchronize(ev));
    }
    if (stats) q->t_wait += host_now() - tw0;
  }
  sl.out_state = 0;
  if (planes) {
    const size_t ysz = (size_t)sl.w * sl.h;
    planes[0] = sl.h_pic;
    planes[1] = sl.h_pic + ysz;
    planes[2] = sl.h_pic + ysz + ysz / 4;
    q->lent = q->head;
  }
  if (strides) {
    strides[0] = sl.w;
    strides[1] = strides[2] = sl.w / 2;
  }
  if (w) *w = sl.w;
  if (h) *h = sl.h;
  if (tag) *tag = sl.tag;
  q->head = (q->head + 1) % q->depth;
  q->count--;
  q->returned++;
  return MI_RTJ_OK;
}

// Kernel times of a session (bench.py's roofline for the in-order workloads): profiling records two events per kernel
// and packet on the submitting thread, so it is switched on for a lap of its own, never inside a timed region.
int mi_rtj_pipe_profile(mi_rtj_pipe* q, int enable) {
  if (!q) return MI_RTJ_ERR_ARG;
  const int rc = mi_rtj_pipe_flush(q);
  if (rc != MI_RTJ_OK) return rc;
  for (auto& sl : q->slot) mi_rtj_plan_profile(sl.plan, enable);
  for (mi_rtj_plan* gp : q->gplan) mi_rtj_plan_profile(gp, enable);
  return MI_RTJ_OK;
}

int mi_rtj_pipe_times(mi_rtj_pipe* q, float ms[MI_RTJ_NUM_KERNELS], int* launches) {
  if (!q || !ms) return MI_RTJ_ERR_ARG;
  pipe_drain_jobs(q);
  int total = 0;
  for (int k = 0; k < MI_RTJ_NUM_KERNELS; k++) ms[k] = 0.f;
  std::vector<mi_rtj_plan*> plans;
  for (auto& sl : q->slot) plans.push_back(sl.plan);
  for (mi_rtj_plan* gp : q->gplan) plans.push_back(gp);
  for (mi_rtj_plan* pl : plans) {  // (launches = k_decode launches = packets: a group's index kernels count once)
    float one[MI_RTJ_NUM_KERNELS];
    int n = 0;
    const int rc = mi_rtj_plan_times(pl, one, &n);
    if (rc != MI_RTJ_OK) return rc;
    for (int k = 0; k < MI_RTJ_NUM_KERNELS; k++) ms[k] += one[k];
    total += n;
  }
  if (launches) *launches = total;
  return MI_RTJ_OK;
}

int mi_rtj_pipe_peek_tag(const mi_rtj_pipe* q, uint64_t* tag) {
  if (!q || !tag || q->count == 0) return MI_RTJ_ERR_ARG;
  *tag = q->slot[q->head].tag;
  return MI_RTJ_OK;
}

int mi_rtj_pipe_flush(mi_rtj_pipe* q) {
  if (!q) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = q->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  // work in flight cannot be recalled; it is waited for and forgotten (a seek is rare, a frame takes microseconds)
  pipe_drain_jobs(q);
  // Packets copied in whose index group was not complete yet are decoded all the same before they are forgotten:
  // q->prev_pic — the picture of the packet submitted last — is then a picture that WAS decoded, and the first packet
  // after the resync takes its unchanged (0xFF) blocks from it, as the reference takes them from priv->frame (ADVICE r3:
  // they used to be dropped unindexed, and prev_pic pointed at a picture up to `depth` packets old or at zeros)
  if (q->nstaged > 0) (void)pipe_issue_staged(q);
  HIPCHK(c, hipStreamSynchronize(q->s_in));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (q->s_idx) HIPCHK(c, hipStreamSynchronize(q->s_idx));
  for (int i = 0; i < q->sw.out_streams; i++) HIPCHK(c, hipStreamSynchronize(q->s_out[i]));
  for (auto& sl : q->slot) {
    sl.out_state = 0;
    sl.staged = 0;
  }
  q->nstaged = 0;
  q->head = (q->head + q->count) % q->depth;
  q->count = 0;
  q->lent = -1;
  return MI_RTJ_OK;
}

}  // extern "C"
