// mi_rtjpeg.hip — host side of libmi_rtjpeg.so: the C ABI of include/mi_rtjpeg.h over the
// gfx950 kernels.  No CPU decode path exists here: without a usable device every entry point
// fails and reports why.
//
// This file: the instance's and a plan's state, plan_launch() and the plan entry points.  The rest of the host layer:
// host_base.h (shared with the other device libraries: owned buffers, streams and events, errors, the bodies of the calls
// every library has), and the rtj_host_*.h headers: pinned memory with flags (rtj_host_buf.h), the environment switches
// (rtj_host_switches.h), the stages of a launch (rtj_host_stages.h), sessions (rtj_host_pipe.h), encoder and colour
// stage (rtj_host_encode.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mi_rtjpeg.h"
#include "rtj_color_kernels.h"
#include "rtj_common.h"
#include "rtj_decode_chroma.h"
#include "rtj_decode_kernels.h"
#include "rtj_encode_kernels.h"
#include "rtj_format_kernels.h"
#include "rtj_index_kernels.h"
#include "rtj_runs_kernels.h"
#include "rtj_spec_kernels.h"
#include "rtj_tables.h"
#include "rtj_walk_kernels.h"
#include "rtj_host_buf.h"
#include "rtj_host_switches.h"

using namespace mirtj;

namespace {

constexpr size_t kAllocPad = 256;  // kernels may read a few bytes past a packet's last dword
constexpr int kMaxPlanFrames = 65535;       // a plan's frames are the y dimension of every grid
constexpr uint64_t kOverlapMaxGroups = 8192ull * 255ull;  // plans from this many macroblock groups on run their kernels back to back

static_assert(MI_RTJ_OK == kOk && MI_RTJ_ERR_HIP == kErrHip, "header and host base agree");

// a kernel's start and end while profiling: handles of events the plan owns (mi_rtj_plan::timing); `a` is the previous
// kernel's `b` where kernels run back to back on one stream
struct Timed {
  hipEvent_t a = nullptr, b = nullptr;
};

// The three picture formats, one row each, indexed by MI_RTJ_FMT_*: the numbers are FmtShape's (rtj_common.h), the
// texts are what the entry points say about the format.  Every size the host derives from a format comes from here.
struct Format {
  uint32_t mb_w, mb_h;  // macroblock, pixels (lib/RTjpeg.c:2651-2653 and 2761-2763 are these loops' steps)
  uint32_t blk_per_mb, parts, units_per_group;
  uint32_t chroma_planes, chroma_sx, chroma_sy;  // chroma planes are (w >> sx) x (h >> sy)
  uint32_t run_tile, run_copy_threads;           // phase 2 of runs: units and lanes of a copy workgroup (RunTile)
  const char* name;
  const char* abi_name;
  const char* header_rule;  // after "packet header WxH: "
  const char* encode_rule;  // after "mi_rtj_encode: WxH: " (4:2:0 has one message for every bad argument)

  bool geometry_ok(int w, int h) const { return w > 0 && h > 0 && w % (int)mb_w == 0 && h % (int)mb_h == 0; }
  uint32_t units_per_row(int w) const { return (uint32_t)w / mb_w; }
  uint64_t units(int w, int h) const { return (uint64_t)units_per_row(w) * ((uint32_t)h / mb_h); }  // macroblocks
  uint64_t blocks(int w, int h) const { return units(w, h) * blk_per_mb; }
  uint32_t groups(uint32_t units) const { return (units + units_per_group - 1u) / units_per_group; }
  size_t chroma_plane_bytes(size_t w, size_t h) const { return chroma_planes ? (w >> chroma_sx) * (h >> chroma_sy) : 0; }
  size_t picture_bytes(size_t w, size_t h) const { return w * h + chroma_planes * chroma_plane_bytes(w, h); }
};
template <int Fmt>
constexpr Format format_row(const char* name, const char* abi_name, const char* header_rule, const char* encode_rule) {
  using S = FmtShape<Fmt>;
  return {S::kMbW, S::kMbH, S::kBlkPerMb, S::kParts, S::kUnitsPerGroup, S::kChromaPlanes, S::kChromaShiftX,
          S::kChromaShiftY, RunTile<Fmt>::kUnits, RunTile<Fmt>::kThreads, name, abi_name, header_rule, encode_rule};
}
constexpr Format kFormats[] = {
    format_row<kFmtYUV420>("4:2:0", "4:2:0 (MI_RTJ_FMT_YUV420)", "width and height must be positive multiples of 16", ""),
    format_row<kFmtYUV422>("4:2:2", "4:2:2 (MI_RTJ_FMT_YUV422)",
                           "a 4:2:2 picture needs a positive width that is a multiple of 16 and a positive height that is a multiple of 8",
                           "a 4:2:2 picture's width is a positive multiple of 16, its height a positive multiple of 8"),
    format_row<kFmtGrey>("greyscale", "greyscale (MI_RTJ_FMT_GREY)",
                         "a greyscale picture needs a positive width and height that are multiples of 8",
                         "a greyscale picture's width and height are positive multiples of 8"),
};
static_assert(MI_RTJ_FMT_YUV420 == kFmtYUV420 && MI_RTJ_FMT_YUV422 == kFmtYUV422 && MI_RTJ_FMT_GREY == kFmtGrey,
              "kFormats is indexed by the ABI's format numbers");
inline bool format_known(int fmt) { return fmt >= 0 && fmt < (int)(sizeof kFormats / sizeof kFormats[0]); }

// ---- a plan's device state, in the groups that are made and freed together (each frees itself) ----

// per-chunk scratch of the exact index.  A group's capacity is read from the buffer allocated last: a group that could
// not be made whole counts as empty.
struct ChunkIndex {
  DevBuf<uint32_t> summary;  // [chunks][kEntries]
  DevBuf<uint16_t> lentab;   // [chunks][kChunk] block lengths (luma | chroma << 8)
  DevBuf<uint32_t> pos, mb;  // [chunks + n]
  uint64_t chunks() const { return lentab.cap / kChunk; }
  uint64_t entries() const { return mb.cap; }
};

// speculative index (rtj_spec_kernels.h): one walker per kSpecChunk bytes, proven per packet afterwards
struct SpecIndex {
  bool on = false;
  uint64_t n = 0;                 // walkers of this plan
  std::vector<SpecChunkDev> h_chunks;
  std::vector<uint32_t> h_base;   // [frames + 1]
  // sized by the walkers
  DevBuf<SpecChunkDev> chunks;
  DevBuf<uint32_t> rec;           // the walkers' start bits: spec_bits_words(walkers) dwords, [wave][tile][lane][4]
  DevBuf<uint32_t> nrec;
  DevBuf<uint32_t> wstart;        // [walkers]: first byte each walker parsed (repairs move it)
  DevBuf<uint2> hand;             // [walkers]: where a chunk takes over / where the next one has to
  DevBuf<uint2> fix;              // [walkers]: (walker, byte to start from) of the chunks to walk again
  DevBuf<uint8_t> flag;           // [walkers + 64]: 1 = on that list in this launch
  DevBuf<uint32_t> nfix;
  // runs of chunks (spec_run_length(); run_s == 1: one walker per chunk and none of these)
  uint32_t run_s = 1;             // chunks a run walker takes at most
  uint64_t nruns = 0;
  std::vector<SpecRunDev> h_runs;
  std::vector<uint32_t> h_rbase;  // [frames + 1]: a packet's first run
  DevBuf<SpecRunDev> runs;        // [nruns]
  DevBuf<uint32_t> rbase;         // [frames + 1]
  DevBuf<uint32_t> runrec;        // the run walkers' start bits: spec_bits_words_t(nruns, spec_run_tiles(run_s)) dwords
  DevBuf<uint32_t> brow;          // [walkers]: whose bits a chunk's are (SpecRunArgs)
  // sized by the frames
  DevBuf<uint32_t> base;          // [frames + 1]
  DevBuf<uint32_t> ok;            // [frames]: 1 = the packet's index is proven
  DevBuf<uint32_t> todo;          // [frames + 2]: count, then the packets left to the exact kernels; [frames + 1]: how many
                                  // of them the serial walker takes instead (k_spec_policy)
  DevBuf<uint32_t> state;         // [kSpecStWords]: launches in a row that refused every packet, launches left paused, ...
  uint64_t walkers_cap() const { return flag.cap; }
  uint64_t frames_cap() const { return todo.cap ? todo.cap - 2 : 0; }
};

// batches: what k_decode_split leaves to k_decode_list (rtj_decode_kernels.h, DecList): every part of every group of a
// launch fits; two counters, launches alternate, a launch's k_decode_list zeroes the other one
struct SplitLists {
  DevBuf<uint2> list;
  DevBuf<uint32_t> cnt;
  // the policy's mode word as the host last saw it: pinned host memory that k_decode_list writes behind its books.  The
  // host reads it without waiting (it may be launches old) for ONE decision: while it says "split form" the classic form's
  // kernel is not enqueued at all (it would return at once: ~90 us of empty workgroups per 16,384 pictures) and
  // k_decode_split is told to run whatever the device's word says — so a stale view costs time on content that just
  // turned noisy, never pictures
  FlagPinnedBuf<uint32_t> h_mode_seen;
  uint32_t* d_mode_seen = nullptr;  // the same word, as the device addresses it
  int flip = 0;
};

// Batches: the index of launch k + 1 is built while launch k is still being transformed.  The only thing the two
// halves of a launch share is the block-offset index, so there are two of those (launches alternate) and an event per
// index that says "k_decode has read it" before the launch after next writes it again.  Both halves are bound by
// vector-instruction issue, so a long launch gains nothing; a short one (1024 pictures: 6 rounds of resident waves
// for k_decode, under one for the walkers) fills the other half's idle tails.  MI_RTJ_OVERLAP=0 / 1 overrides.
struct Overlap {
  bool on = false;
  // Long launches (which do not overlap by default) of NOISY content do gain: there the index is the serial walker, heavy
  // on the scalar unit, next to a transform heavy on the vector unit (+-32: 332 K against 297 K pictures per second at
  // 16,384 per launch, +-64: 271 K against 251 K, profiles/r04/overlap_at_16384.txt).  The host knows such content by
  // the decode policy's mode word (h_mode_seen: "classic form"), seen without waiting; while it says so the launches of
  // a plan that may (dyn) run like an overlapped plan's; the second index and the stream are made with the plan.
  bool dyn = false;
  bool last_overlapped = false;  // the launch before this one ran its index on own_idx
  // (members are destroyed last to first: the events and the second index before the stream, which is waited for first)
  Stream own_idx;
  DevBuf<uint32_t> blkoff_b;     // the second block-offset index (the plan's blkoff is the first)
  Event e_read[2];
  Event e_idx;                   // index done (used whenever the index kernels have a stream of their own)
  int flip = 0;                  // which index the NEXT launch writes
  int last = 0;                  // which one the last launch wrote (mi_rtj_plan_read_index)

  void drop_stream() {
    if (own_idx) (void)hipStreamSynchronize(own_idx);
    own_idx.release();
  }
  ~Overlap() {
    if (own_idx) (void)hipStreamSynchronize(own_idx);
  }
};

// Runs (mi_rtj_plan_set_runs / _fmt, rtj_runs_kernels.h): phase 2 resolves the unchanged blocks of pictures k > 0 of a
// run behind the transform.  Everything is made by set_runs; a launch only queues the three kernels of the plan's format.
struct Runs {
  int n_runs = 0;                    // runs as set (0: independent pictures)
  uint32_t list = 0, chunks = 0;     // runs of two or more pictures / their chunks: what phase 2 covers
  uint32_t nmb_max = 0;
  DevBuf<RunDev> d_runs;
  DevBuf<RunChunkDev> d_chunks;
  DevBuf<uint64_t> d_mask;           // [chunk][block]: pictures of the chunk that code the block
  DevBuf<uint16_t> d_carry;          // [chunk][block]: run-relative source of the chunk's first picture
  DevBuf<unsigned long long> d_copied;  // unchanged blocks copied by the last launch
};

}  // namespace

// Device, stream and error text are HostCtx's (host_base.h), destroyed after everything here: buffers and e_input go
// before the stream.
struct mi_rtj_ctx : HostCtx {
  DevBuf<QTab> d_lut;
  uint8_t b8[kNumQTab][2] = {};  // host copy of (lb8, cb8) per LUT row
  // RTjpeg_t's header-driven state (lib/RTjpeg.c:3568-3579)
  int width = 0, height = 0, Q = 0;
  // which arm of RTjpeg_decompress's switch the instance decodes (RTjpeg_set_format, lib/RTjpeg.c:2421): MI_RTJ_FMT_*.
  // Fixed by the first decode, plan or session: the persistent picture below has one layout.
  int fmt = 0;
  bool fmt_fixed = false;
  DevBuf<uint8_t> d_frame;        // persistent picture of the one-packet path (priv->frame of lib/video_rtjpeg.c:31-35)
  DevBuf<uint8_t> d_pkt;
  PinnedBuf<uint8_t> h_frame;     // pinned host picture of the nocopy path
  mi_rtj_plan* single = nullptr;  // reusable 1-frame plan
  // Asynchronous producers on the instance's stream (mi_rtj_dev_memset) may have written what a plan's index kernels
  // read on their own stream: the next launch of a plan with an index stream makes that stream wait for this event once
  // (not at every launch — that would put the index of launch k + 1 behind the transform of launch k)
  bool input_dirty = false;
  Event e_input;
};

struct mi_rtj_plan {
  mi_rtj_ctx* ctx = nullptr;
  int n = 0;
  int fmt = 0;                      // the instance's format when the plan was made (MI_RTJ_FMT_*)
  PlanSwitches sw;                  // the environment switches this kind of plan honours (rtj_host_switches.h)
  std::vector<FrameDev> h_frames;
  DevBuf<FrameDev> own_frames;      // the descriptors of a plan that uploads its own (batches, the one-packet plan)
  const FrameDev* d_frames = nullptr;  // what the kernels read: own_frames, or a session's staging / descriptor array
  DevBuf<uint32_t> blkoff;          // the block-offset index
  uint64_t n_blocks = 0, n_index = 0, bytes_in = 0, bytes_out = 0;  // n_index: entries of the index the frames use
  uint32_t max_groups = 0, max_chunks = 0;
  bool profile = false;
  bool one_block_type = false;      // every frame's tables have lb8 == cb8: single-search summarize
  bool batch_seen = false;          // a batch launch (a wave takes several parts of its groups, no previous picture) was queued
  const uint8_t* prev_pic = nullptr;  // sessions: where unchanged blocks of this launch are copied from
  hipStream_t idx_stream = nullptr;   // the stream of the index kernels (sessions: theirs, not owned; batches: ov.own_idx); null = the instance's
  ChunkIndex chunk;
  SpecIndex spec;
  SplitLists split;
  Runs runs;
  bool runs_ran = false;            // the last launch ran phase 2
  Overlap ov;                       // (declared behind the buffers: its stream is waited for before any of them is freed)
  std::vector<Timed> ev[MI_RTJ_NUM_KERNELS];  // one pair per launch while profiling
  std::vector<Timed> run_ev;        // while profiling: one per launch (b == nullptr: no phase 2 in it)
  std::vector<Event> timing;        // the events ev and run_ev name (behind ov: they go before its stream)
  int launches = 0;
};

namespace {

// RTjpeg_decompress's header handling (lib/RTjpeg.c:3568-3579) on the instance state.
// Returns the LUT row to use, or a negative error.
int apply_header(mi_rtj_ctx* c, const uint8_t* hdr, int* w, int* h) {
  const int hw = hdr[6] | (hdr[7] << 8), hh = hdr[8] | (hdr[9] << 8), q = hdr[10];
  const Format& F = kFormats[c->fmt];
  if (!F.geometry_ok(hw, hh)) return fail(c, MI_RTJ_ERR_GEOMETRY, "packet header %dx%d: %s", hw, hh, F.header_rule);
  c->width = hw;
  c->height = hh;
  if (q != c->Q) c->Q = q < 1 ? 1 : q;  // RTjpeg_set_quality clamps to 1..255 (lib/RTjpeg.c:2410-2411)
  *w = hw;
  *h = hh;
  return c->Q;  // 0 only while no non-zero quality was ever seen: the all-zero tables
}

int fill_frame(mi_rtj_ctx* c, const uint8_t* hdr, uint64_t pkt_off, uint32_t pkt_len, uint64_t out_off,
               uint32_t blk_base, FrameDev* f) {
  int w, h;
  const int q = apply_header(c, hdr, &w, &h);
  if (q < 0) return q;
  if (out_off & 15) return fail(c, MI_RTJ_ERR_ARG, "out_offset %llu is not a multiple of 16", (unsigned long long)out_off);
  memset(f, 0, sizeof(*f));
  f->data_off = pkt_off + MI_RTJ_HEADER_SIZE;
  f->out_off = out_off;
  if (pkt_len >= 0x80000000u) return fail(c, MI_RTJ_ERR_ARG, "packet of %u bytes: packets are limited to 2 GiB", pkt_len);
  f->data_len = pkt_len > MI_RTJ_HEADER_SIZE ? pkt_len - MI_RTJ_HEADER_SIZE : 0;
  f->w = (uint32_t)w;
  f->h = (uint32_t)h;
  f->qidx = (uint32_t)q;
  f->blk_base = blk_base;
  const Format& F = kFormats[c->fmt];
  f->mbw = F.units_per_row(w);
  f->nmb = (uint32_t)F.units(w, h);  // (a header's 16-bit sizes: at most 2^26 units)
  if (F.blocks(w, h) * 64 + kAllocPad >= 0xFFFFFFFFull)  // block offsets and the walkers' positions are 32-bit
    return fail(c, MI_RTJ_ERR_GEOMETRY, "picture of %dx%d: its worst-case stream does not fit 32-bit offsets", w, h);
  f->nchunks = (f->data_len + kChunk - 1) / kChunk;
  if (f->nchunks == 0) f->nchunks = 1;
  return MI_RTJ_OK;
}

// blocks, macroblock groups and plane bytes of a picture in the plan's format
inline uint64_t frame_blocks(const FrameDev& f, int fmt) { return (uint64_t)f.nmb * kFormats[fmt].blk_per_mb; }
inline uint32_t frame_groups(const FrameDev& f, int fmt) { return kFormats[fmt].groups(f.nmb); }
inline size_t frame_plane_bytes(const FrameDev& f, int fmt) { return kFormats[fmt].picture_bytes(f.w, f.h); }
// entries a picture takes in the block index: one per block and the end, rounded so that every picture's part is
// 256-byte aligned
inline uint64_t frame_index_entries(const FrameDev& f, int fmt) { return ((frame_blocks(f, fmt) + 1) + 63) & ~63ull; }

// a plan of `n` packets in the instance's format, with the switches its kind honours; nothing on the device yet
mi_rtj_plan* plan_new(mi_rtj_ctx* c, int n, PlanKind kind) {
  mi_rtj_plan* p = new mi_rtj_plan();
  p->ctx = c;
  p->n = n;
  p->fmt = c->fmt;
  p->sw = plan_switches_from_env(kind);
  p->h_frames.resize((size_t)n);
  return p;
}

// room for `entries` in the block index; a plan that has to grow takes `capacity_hint` if that is more (sessions: room
// for a whole group).  Work in flight on the instance's stream is waited for before the old index goes.
int plan_fit_index(mi_rtj_plan* p, uint64_t entries, uint64_t capacity_hint) {
  p->n_index = entries;
  if (entries <= p->blkoff.cap) return MI_RTJ_OK;
  return p->blkoff.grow(p->ctx, std::max(entries, capacity_hint), p->ctx->stream);
}

// per-chunk scratch of a plan (re)sized for its frames; chunk_base / sum_base are set here
int plan_alloc_chunks(mi_rtj_plan* p) {
  mi_rtj_ctx* c = p->ctx;
  hipStream_t const s = c->stream;
  uint64_t chunks = 0, entries = 0;
  p->max_chunks = 0;
  p->one_block_type = true;
  for (auto& f : p->h_frames) {
    p->one_block_type = p->one_block_type && c->b8[f.qidx][0] == c->b8[f.qidx][1];
    f.sum_base = (uint32_t)chunks;
    f.chunk_base = (uint32_t)entries;
    chunks += f.nchunks;
    entries += f.nchunks + 1;
    if (f.nchunks > p->max_chunks) p->max_chunks = f.nchunks;
  }
  ChunkIndex& ch = p->chunk;
  int rc;  // (MI_RTJ_OK is 0: the first step of a chain that fails ends it)
  if (chunks > ch.chunks() && ((rc = release_together(c, s, ch.summary, ch.lentab)) || (rc = ch.summary.grow(c, kEntries * chunks, s)) ||
                               (rc = ch.lentab.grow(c, kChunk * chunks, s, 64))))
    return rc;
  if (entries > ch.entries() && ((rc = release_together(c, s, ch.pos, ch.mb)) || (rc = ch.pos.grow(c, entries, s)) || (rc = ch.mb.grow(c, entries, s))))
    return rc;
  // ---- speculative index: worth it once the batch fills the device (a walker is one lane and runs
  //      for ~0.25 ms whatever the batch; a single packet is indexed faster by the exact kernels) ----
  SpecIndex& sp = p->spec;
  uint64_t walkers = 0;
  // one walker per kSpecChunk bytes AND one whose chunk begins at or past the packet's last byte: the index's last entry,
  // the end position, is the start of a block that is not there, and a packet whose length is a whole number of chunks
  // has it at the first byte of a chunk of its own (12 of the bench's 16,384 packets were refused for the lack of it)
  auto spec_chunks_of = [](const FrameDev& f) -> uint32_t { return f.data_len / (uint32_t)kSpecChunk + 1u; };
  for (auto& f : p->h_frames) walkers += spec_chunks_of(f);
  sp.on = !p->sw.serial_index && !p->sw.emit_walk && (p->sw.spec_mode >= 1 || (p->sw.spec_mode != 0 && walkers >= kSpecMinWalkers));
  if (sp.on) {
    sp.h_chunks.clear();
    sp.h_base.assign(1, 0u);
    for (size_t i = 0; i < p->h_frames.size(); i++) {
      const uint32_t nsc = spec_chunks_of(p->h_frames[i]);
      for (uint32_t k = 0; k < nsc; k++) sp.h_chunks.push_back(SpecChunkDev{(uint32_t)i, k});
      sp.h_base.push_back((uint32_t)sp.h_chunks.size());
    }
    sp.n = sp.h_chunks.size();
    if (sp.n >= 0x7FFFFFFFull) sp.on = false;  // walker numbers are 32-bit
  }
  if (!sp.on) return MI_RTJ_OK;
  // runs: the short lead only (plans forced to a longer one keep a walker per chunk), by the number of chunks or
  // MI_RTJ_SPEC_RUN; plans whose blocks all parse alike (lb8 == cb8, the 10-instruction byte step) take them only when forced
  sp.run_s = p->sw.spec_mode == 3 || p->sw.spec_mode == 4 || (p->one_block_type && p->sw.spec_run < 1)
                 ? 1u
                 : spec_run_length(sp.n, p->sw.spec_run);
  sp.h_runs.clear();
  sp.h_rbase.assign(1, 0u);
  if (sp.run_s > 1u)
    for (size_t i = 0; i < p->h_frames.size(); i++) {
      spec_packet_runs((uint32_t)i, sp.h_base[i], sp.h_base[i + 1] - sp.h_base[i], sp.run_s, sp.h_runs);
      sp.h_rbase.push_back((uint32_t)sp.h_runs.size());
    }
  sp.nruns = sp.h_runs.size();
  const uint64_t frames = p->h_frames.size();
  // (rec: whole waves of walkers, + a spare walker for idle lanes; flag: the walkers zero [0, n) per launch; nfix and, below,
  // state are made once; ok starts as "nothing proven yet" for mi_rtj_plan_spec_stats)
  if (sp.n > sp.walkers_cap() &&
      ((rc = release_together(c, s, sp.chunks, sp.rec, sp.nrec, sp.wstart, sp.hand, sp.fix, sp.flag)) || (rc = sp.chunks.grow(c, sp.n, s)) ||
       (rc = sp.rec.grow(c, spec_bits_words(sp.n), s)) || (rc = sp.nrec.grow(c, sp.n, s)) || (rc = sp.wstart.grow(c, sp.n, s)) ||
       (rc = sp.hand.grow(c, sp.n, s)) || (rc = sp.fix.grow(c, sp.n, s)) || (rc = sp.flag.grow(c, sp.n, s, 64, true)) ||
       (rc = sp.nfix.grow(c, 1, s, 0, true))))
    return rc;
  if (frames > sp.frames_cap()) {
    if ((rc = release_together(c, s, sp.base, sp.ok, sp.todo)) || (rc = sp.base.grow(c, frames + 1, s)) || (rc = sp.ok.grow(c, frames, s, 0, true)) ||
        (rc = sp.todo.grow(c, frames + 2, s)))
      return rc;
    HIPCHK(c, hipMemsetAsync(sp.todo + frames + 1, 0, sizeof(uint32_t), s));
    if ((rc = sp.state.grow(c, kSpecStWords, s, 0, true))) return rc;
  }
  if (sp.run_s > 1u) {
    const uint64_t words = spec_bits_words_t(sp.nruns, spec_run_tiles(sp.run_s));
    if ((sp.nruns > sp.runs.cap && ((rc = release_together(c, s, sp.runs)) || (rc = sp.runs.grow(c, sp.nruns, s)))) ||
        (words > sp.runrec.cap && ((rc = release_together(c, s, sp.runrec)) || (rc = sp.runrec.grow(c, words, s)))) ||
        (sp.n > sp.brow.cap && ((rc = release_together(c, s, sp.brow)) || (rc = sp.brow.grow(c, sp.n, s)))) ||
        (sp.h_rbase.size() > sp.rbase.cap && ((rc = release_together(c, s, sp.rbase)) || (rc = sp.rbase.grow(c, sp.h_rbase.size(), s)))))
      return rc;
    HIPCHK(c, hipMemcpyAsync(sp.rbase, sp.h_rbase.data(), sizeof(uint32_t) * sp.h_rbase.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(sp.runs, sp.h_runs.data(), sizeof(SpecRunDev) * sp.nruns, hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, hipMemcpyAsync(sp.chunks, sp.h_chunks.data(), sizeof(SpecChunkDev) * sp.n, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(sp.base, sp.h_base.data(), sizeof(uint32_t) * sp.h_base.size(), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));  // the host vectors may be rebuilt by the next call
  return MI_RTJ_OK;
}

// the descriptors of a plan that owns them, on their way to the device
int plan_upload(mi_rtj_plan* p) {
  mi_rtj_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = p->own_frames.grow(c, (uint64_t)p->n, c->stream);
  if (rc != MI_RTJ_OK) return rc;
  p->d_frames = p->own_frames;
  HIPCHK(c, hipMemcpyAsync(p->own_frames, p->h_frames.data(), sizeof(FrameDev) * p->n, hipMemcpyHostToDevice, c->stream));
  return MI_RTJ_OK;
}

// what: the index kernels (kLaunchIndex), k_decode (kLaunchDecode) or both.  A session whose packets are indexed in
// groups queues the index of a group once and then k_decode packet by packet (dframe = the packet's place in the group,
// dcount = 1, d_out = its picture): a packet's unchanged blocks come from its predecessor's picture, so the pictures of
// a group cannot be made by one launch.
enum { kLaunchIndex = 1, kLaunchDecode = 2, kLaunchAll = 3 };

}  // namespace

#include "rtj_host_stages.h"

namespace {

// phase 2's grids from the format's block and tile counts (rtj_runs_kernels.h): a lane per block of the largest picture
// for the scans, a workgroup per tile of units (4:2:0 and 4:2:2: 32 macroblocks, greyscale: 64 blocks) for the copy
RunGrids run_grids(const mi_rtj_plan* p) {
  const Runs& r = p->runs;
  const Format& F = kFormats[p->fmt];
  const unsigned bx = (unsigned)(((uint64_t)F.blk_per_mb * r.nmb_max + kRunScanThreads - 1) / kRunScanThreads);
  RunGrids rg;
  rg.copy_threads = F.run_copy_threads;
  rg.items = r.chunks * (uint32_t)kRunSubs;
  rg.mask = dim3(bx, std::min(r.chunks, kRunMaxGridY));
  rg.carry = dim3(bx, std::min(r.list, kRunMaxGridY));
  rg.copy = dim3((r.nmb_max + F.run_tile - 1) / F.run_tile, std::min(rg.items, kRunMaxGridY));
  return rg;
}

// The stages are rtj_host_stages.h's, called in order; everything that sizes a grid is here.
int plan_launch(mi_rtj_plan* p, const void* d_stream, void* d_out, int what = kLaunchAll, uint32_t dframe = 0,
                int dcount = -1) {
  mi_rtj_ctx* c = p->ctx;
  Launch L(p, (const uint8_t*)d_stream);
  if (p->fmt != MI_RTJ_FMT_YUV420)  // the serial index, a wave per packet, then the transform, then phase 2 of runs
    return launch_fmt(L, dim3(std::min<unsigned>((unsigned)p->n, 16384u)),
                      dim3(kFormats[p->fmt].parts * p->max_groups, (unsigned)p->n), p->runs.chunks > 0, run_grids(p),
                      (uint8_t*)d_out);
  int rc;
  if ((rc = launch_open(L, what)) != MI_RTJ_OK) return rc;
  if (what & kLaunchIndex) {
    unsigned rows = (unsigned)p->n;  // grid rows of the exact kernels: one per packet, or a few that loop over the to-do list
    const bool spec = p->spec.on && !p->sw.serial_index;
    if (spec) {
      rows = std::min<unsigned>(rows, kSpecFallbackRows);
      // a lane per chunk, or per run where nothing but the short lead can be asked for (with a policy the longer leads
      // still walk a lane per chunk, and the policy's choice is the device's to know: k_spec_walk_any)
      const int sm = p->sw.spec_mode;
      const uint64_t lanes = p->spec.run_s > 1u && sm == 1 ? p->spec.nruns : p->spec.n;
      const SpecGrids g{dim3((unsigned)((lanes + 63) / 64)), dim3(p->n), dim3(kSpecRepairGrid)};
      if ((rc = stage_spec_index(L, g)) != MI_RTJ_OK) return rc;
    }
    ExactGrids g;
    g.walk = dim3(p->n);
    g.walk_todo = dim3(std::min<unsigned>((unsigned)p->n, 16384u));
    g.summarize = dim3(p->max_chunks, rows);
    g.resolve = dim3(spec ? std::min<unsigned>((unsigned)p->n, 1024u) : rows);
    g.emit = p->sw.emit_walk ? dim3(p->max_chunks, p->n) : dim3(p->max_chunks, rows);
    if ((rc = stage_exact_index(L, g)) != MI_RTJ_OK) return rc;
  }
  if ((rc = launch_hand_over(L, what)) != MI_RTJ_OK) return rc;
  if (!(what & kLaunchDecode)) {
    HIPCHK(c, hipGetLastError());
    return MI_RTJ_OK;
  }
  const unsigned drows = dcount < 0 ? (unsigned)p->n : (unsigned)dcount;
  // the A/B override is honoured only where it still covers every group
  // a wave per (slot, part) or, in batches that still make enough waves that way, per slot: the wave then takes the
  // three parts of each of its groups in turn and the group's stream bytes cross the fabric once (kernel header)
  const uint32_t span = p->sw.rotate >= 0 ? (p->sw.rotate ? 3u : 1u)
                        : (uint64_t)drows * p->max_groups >= (uint64_t)kDecRotateMinGroups ? 3u : 1u;
  const uint32_t dslots = p->sw.dec_slots && p->sw.dec_slots * (uint32_t)kDecIters >= p->max_groups
                              ? p->sw.dec_slots
                              : decode_slots(p->max_groups, (uint32_t)drows, span);
  const dim3 grid(span == 3u ? dslots : dslots * 3u, drows), block(kDecThreads);
  const Transform T{p->d_frames + dframe, (uint8_t*)d_out, grid, block};
  if (span == 3u && !p->prev_pic) p->batch_seen = true;
  if (span == 3u && !p->prev_pic && p->sw.split != 0) {
    const uint64_t need = 3ull * drows * p->max_groups;  // the list takes every part of every group
    if ((rc = ensure_split_lists(p, need)) != MI_RTJ_OK) return rc;
    uint32_t lw = split_luma_waves(p->max_groups);
    uint32_t cw = split_chroma_waves(p->max_groups);
    const LaunchExperiments x = launch_experiments_from_env(kSplitXcdRot);
    if (x.luma_waves) lw = x.luma_waves;
    if (x.chroma_waves) cw = x.chroma_waves;
    if (x.split_only) (x.split_only == 1 ? cw : lw) = 0u;  // (timing builds only, wrong pictures: one kind of wave alone)
    rc = stage_transform_split(L, T, dim3(kXcds * (lw + cw), drows), dim3(kDecListGrid), lw, cw, x, need);
  } else {
    rc = stage_transform_classic(L, T, span == 3u);
  }
  if (rc != MI_RTJ_OK) return rc;
  const bool runs = what == kLaunchAll && p->runs.chunks > 0;
  if ((rc = stage_runs(L, runs, run_grids(p), (uint8_t*)d_out)) != MI_RTJ_OK) return rc;
  return launch_close(L, what, runs);
}

}  // namespace

extern "C" {

int mi_rtj_device_count(void) { return device_count(); }

mi_rtj_ctx* mi_rtj_create(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    fail(nullptr, MI_RTJ_ERR_NO_DEVICE, "no HIP device: %s — this library has no CPU path", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  if (device >= n) {
    fail(nullptr, MI_RTJ_ERR_ARG, "device %d out of range (%d devices)", device, n);
    return nullptr;
  }
  if (!is_gfx950(device)) {
    hipDeviceProp_t p;
    (void)hipGetDeviceProperties(&p, device);
    fail(nullptr, MI_RTJ_ERR_NO_DEVICE, "device %d is %s; the kernels are built for gfx950 only", device, p.gcnArchName);
    return nullptr;
  }
  mi_rtj_ctx* c = new mi_rtj_ctx();
  c->device = device;
  auto bail = [&](const char* what, hipError_t err) -> mi_rtj_ctx* {
    fail(nullptr, MI_RTJ_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
    mi_rtj_destroy(c);
    return nullptr;
  };
  if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
  if ((e = hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
  std::vector<QTab> lut(kNumQTab);
  build_all_qtabs(lut.data());
  for (int q = 0; q < kNumQTab; q++) {
    c->b8[q][0] = (uint8_t)lut[q].lb8;
    c->b8[q][1] = (uint8_t)lut[q].cb8;
    // k_decode places DC and the raw bytes inside a block's first 16 bytes (the formula yields 0, 4, 8, 9)
    if (lut[q].lb8 > kMaxRawBytes || lut[q].cb8 > kMaxRawBytes) {
      fail(nullptr, MI_RTJ_ERR_ARG, "quantiser table %d has more than %d raw coefficients", q, kMaxRawBytes);
      mi_rtj_destroy(c);
      return nullptr;
    }
  }
  if (c->d_lut.grow(c, kNumQTab, c->stream) != MI_RTJ_OK) return bail("hipMalloc(lut)", hipErrorOutOfMemory);
  if ((e = hipMemcpy(c->d_lut, lut.data(), sizeof(QTab) * kNumQTab, hipMemcpyHostToDevice)) != hipSuccess)
    return bail("hipMemcpy(lut)", e);
  return c;
}

void mi_rtj_destroy(mi_rtj_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->single) mi_rtj_plan_destroy(c->single);
  delete c;  // (buffers and e_input, then HostCtx's stream)
}

const char* mi_rtj_last_error(const mi_rtj_ctx* c) { return last_error(c); }

int mi_rtj_set_format(mi_rtj_ctx* c, int fmt) {
  if (!c) return MI_RTJ_ERR_ARG;
  if (!format_known(fmt))
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_set_format: unknown format %d (0 = 4:2:0, 1 = 4:2:2, 2 = greyscale)", fmt);
  if (c->fmt_fixed && fmt != c->fmt)
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_set_format: the instance has decoded, planned or opened a session in format %d; "
                "its persistent picture has that layout (make a new instance for format %d)", c->fmt, fmt);
  c->fmt = fmt;
  return MI_RTJ_OK;
}

int mi_rtj_get_format(const mi_rtj_ctx* c) { return c ? c->fmt : MI_RTJ_ERR_ARG; }

void mi_rtj_get_state(const mi_rtj_ctx* c, int* w, int* h, int* q) {
  if (!c) return;
  if (w) *w = c->width;
  if (h) *h = c->height;
  if (q) *q = c->Q;
}

void* mi_rtj_dev_alloc(mi_rtj_ctx* c, size_t bytes) {
  if (!c) return nullptr;
  void* p = nullptr;
  if (hipSetDevice(c->device) != hipSuccess) return nullptr;
  hipError_t e = hipMalloc(&p, bytes + kAllocPad);
  if (e != hipSuccess) {
    fail(c, MI_RTJ_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return nullptr;
  }
  // the tail pad is read (never used) by dword-granular staging; keep it defined
  (void)hipMemsetAsync((uint8_t*)p + bytes, 0, kAllocPad, c->stream);
  return p;
}

void mi_rtj_dev_free(mi_rtj_ctx* c, void* d) { dev_free(c, d); }

int mi_rtj_h2d(mi_rtj_ctx* c, void* d, const void* s, size_t n) {
  if (!c || (!d && n) || (!s && n)) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_h2d: NULL argument");
  return copy_sync(c, d, s, n, hipMemcpyHostToDevice);
}

int mi_rtj_d2h(mi_rtj_ctx* c, void* dst, const void* d, size_t n) {
  if (!c || (!d && n) || (!dst && n)) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_d2h: NULL argument");
  return copy_sync(c, dst, d, n, hipMemcpyDeviceToHost);
}

int mi_rtj_dev_memset(mi_rtj_ctx* c, void* d, int v, size_t n) {
  if (!c || (!d && n)) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_dev_memset: NULL argument");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(d, v, n, c->stream));
  c->input_dirty = true;  // (plans whose index kernels run on another stream wait for it: launch_open)
  return MI_RTJ_OK;
}

int mi_rtj_sync(mi_rtj_ctx* c) { return c ? stream_sync(c) : MI_RTJ_ERR_ARG; }

mi_rtj_plan* mi_rtj_plan_create(mi_rtj_ctx* c, int n, const uint8_t* headers, const uint64_t* pkt_offset,
                                const uint32_t* pkt_len, const uint64_t* out_offset) {
  if (!c || n <= 0 || !headers || !pkt_offset || !pkt_len || !out_offset) {
    fail(c, MI_RTJ_ERR_ARG, "mi_rtj_plan_create: bad argument");
    return nullptr;
  }
  if (n > kMaxPlanFrames) {
    fail(c, MI_RTJ_ERR_ARG, "mi_rtj_plan_create: %d packets; a plan takes at most %d (split the batch)", n, kMaxPlanFrames);
    return nullptr;
  }
  mi_rtj_plan* p = plan_new(c, n, kPlanBatch);
  auto refuse = [&]() -> mi_rtj_plan* {
    mi_rtj_plan_destroy(p);
    return nullptr;
  };
  uint64_t blk_base = 0;
  for (int i = 0; i < n; i++) {
    if (blk_base > 0xFFFFFFFFull - (1u << 24)) {
      fail(c, MI_RTJ_ERR_ARG, "plan too large: block index exceeds 32 bits");
      delete p;
      return nullptr;
    }
    if (fill_frame(c, headers + (size_t)i * MI_RTJ_HEADER_SIZE, pkt_offset[i], pkt_len[i], out_offset[i],
                   (uint32_t)blk_base, &p->h_frames[i]) != MI_RTJ_OK) {
      delete p;
      return nullptr;
    }
    const FrameDev& f = p->h_frames[i];
    p->n_blocks += frame_blocks(f, p->fmt);
    blk_base += frame_index_entries(f, p->fmt);
    p->bytes_in += pkt_len[i];
    p->bytes_out += frame_plane_bytes(f, p->fmt);
    p->max_groups = std::max(p->max_groups, frame_groups(f, p->fmt));
  }
  // (a 4:2:2 or greyscale plan has the serial index only: no chunk scratch, no speculation)
  if (hipSetDevice(c->device) != hipSuccess || (p->fmt == MI_RTJ_FMT_YUV420 && plan_alloc_chunks(p) != MI_RTJ_OK)) return refuse();
  if (plan_fit_index(p, blk_base, 0) != MI_RTJ_OK) {
    fail(c, MI_RTJ_ERR_NOMEM, "hipMalloc(block index, %llu entries) failed", (unsigned long long)p->n_index);
    return refuse();
  }
  {
    // by default for plans of 129 .. 8191 pictures of 1080p: smaller ones do not fill the device either way and pay for
    // the cross-stream waits; longer launches gain under 1 % (profiles/r03/ab_overlap_index_with_transform.txt), and
    // kernels that share the device cannot be timed one by one — the per-kernel figures of bench.py and rocprofv3 are
    // taken on launches that run their kernels back to back
    Overlap& o = p->ov;
    const uint64_t groups = (uint64_t)p->n * p->max_groups;
    o.on = p->sw.overlap_set ? p->sw.overlap == 1 : groups >= (uint64_t)kDecRotateMinGroups && groups < (uint64_t)kOverlapMaxGroups;
    o.dyn = p->sw.overlap_set ? p->sw.overlap == 2 : !o.on && groups >= (uint64_t)kOverlapMaxGroups;  // (2: tests, on small plans)
    if (p->fmt != MI_RTJ_FMT_YUV420) o.on = o.dyn = false;  // both kernels on the instance's stream
    if ((o.on || o.dyn) && (o.blkoff_b.grow(c, p->n_index, c->stream) != MI_RTJ_OK ||
                            hipStreamCreateWithFlags(&o.own_idx.p, hipStreamNonBlocking) != hipSuccess)) {
      if (o.on) {
        fail(c, MI_RTJ_ERR_NOMEM, "second block index / index stream of the plan");
        return refuse();
      }
      (void)hipGetLastError();  // wanted, not needed: a plan without room for the second index stays as it was
      o.blkoff_b.release();
      o.drop_stream();
      o.dyn = false;
    }
    if (o.on) p->idx_stream = o.own_idx;
  }
  if (plan_upload(p) != MI_RTJ_OK) return refuse();
  if (p->ov.on && hipStreamSynchronize(c->stream) != hipSuccess) return refuse();  // the descriptors are read from the other stream too
  c->fmt_fixed = true;
  return p;
}

void mi_rtj_plan_destroy(mi_rtj_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  delete p;  // (its events and every group of its state free themselves)
}

int mi_rtj_plan_decode(mi_rtj_plan* p, const void* d_stream, void* d_out) {
  if (!p || !d_stream || !d_out) return fail(p ? p->ctx : nullptr, MI_RTJ_ERR_ARG, "mi_rtj_plan_decode: NULL argument");
  HIPCHK(p->ctx, hipSetDevice(p->ctx->device));
  return plan_launch(p, d_stream, d_out);
}

void mi_rtj_plan_info(const mi_rtj_plan* p, int* n, uint64_t* nb, uint64_t* bi, uint64_t* bo) {
  if (!p) return;
  if (n) *n = p->n;
  if (nb) *nb = p->n_blocks;
  if (bi) *bi = p->bytes_in;
  if (bo) *bo = p->bytes_out;
}

void mi_rtj_plan_profile(mi_rtj_plan* p, int enable) {
  if (!p) return;
  (void)hipStreamSynchronize(p->ctx->stream);
  for (auto& v : p->ev) v.clear();
  p->run_ev.clear();
  p->timing.clear();
  p->profile = enable != 0;
  p->launches = 0;
}

int mi_rtj_plan_times(mi_rtj_plan* p, float ms[MI_RTJ_NUM_KERNELS], int* launches) {
  if (!p || !ms) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = p->ctx;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < MI_RTJ_NUM_KERNELS; k++) {
    ms[k] = 0.f;
    for (auto& t : p->ev[k]) {
      float x = 0;
      HIPCHK(c, hipEventElapsedTime(&x, t.a, t.b));
      ms[k] += x;
    }
  }
  if (launches) *launches = (int)p->ev[MI_RTJ_K_DECODE].size();
  return MI_RTJ_OK;
}

int mi_rtj_plan_step_times(mi_rtj_plan* p, float* ms, int max_steps, int* steps) {
  if (!p || !ms || !steps || max_steps < 0) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = p->ctx;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int n = (int)p->ev[MI_RTJ_K_DECODE].size();
  *steps = n;
  for (int i = 0; i < n && i < max_steps; i++) {
    // the kernel whose begin event is no kernel's end event is the first of its launch; k_decode's end event closes the launch.
    // (This takes entry i of every kernel's list to be launch i: true of a plan whose launches all run the same stages,
    // which the plans this call is made for — batches, kLaunchAll — do)
    auto ends_a_kernel = [&](hipEvent_t e) {
      for (const auto& v : p->ev)
        if ((int)v.size() > i && v[i].b == e) return true;
      return false;
    };
    hipEvent_t first = nullptr;
    for (int k = 0; k < MI_RTJ_NUM_KERNELS && !first; k++)
      if ((int)p->ev[k].size() > i && !ends_a_kernel(p->ev[k][i].a)) first = p->ev[k][i].a;
    // (a launch with runs ends with phase 2)
    hipEvent_t last = (int)p->run_ev.size() > i && p->run_ev[i].b ? p->run_ev[i].b : p->ev[MI_RTJ_K_DECODE][i].b;
    float x = 0;
    if (first) HIPCHK(c, hipEventElapsedTime(&x, first, last));
    ms[i] = x;
  }
  return MI_RTJ_OK;
}

int mi_rtj_plan_spec_lead(mi_rtj_plan* p, int* lead_bytes, int* paused_launches) {
  if (!p || !lead_bytes || !paused_launches) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = p->ctx;
  const int mode = p->sw.spec_mode;
  *lead_bytes = 0;
  *paused_launches = 0;
  if (!p->spec.on) return MI_RTJ_OK;
  *lead_bytes = mode == 4 ? kSpecLeadVery : mode == 3 ? kSpecLeadLong : kSpecLead;
  if (mode == 1 || mode == 3 || mode == 4 || !p->spec.state) return MI_RTJ_OK;  // no policy
  uint32_t st[kSpecStWords];
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(st, p->spec.state, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *lead_bytes = spec_lead_of_level(st[kSpecStLong]);
  *paused_launches = (int)st[kSpecStPause];
  return MI_RTJ_OK;
}

int mi_rtj_plan_overlapped(const mi_rtj_plan* p) { return p && p->ov.last_overlapped ? 1 : 0; }

int mi_rtj_plan_decode_form(mi_rtj_plan* p, int* form, int* classic_launches_left, long long* parts_listed) {
  if (!p || !form || !classic_launches_left || !parts_listed) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = p->ctx;
  const int split = p->sw.split;
  *form = -1;  // no batch launch yet, or a plan whose launches are not batches: k_decode's other forms
  *classic_launches_left = 0;
  *parts_listed = 0;
  if (!p->batch_seen) return MI_RTJ_OK;
  if (split == 0 || !p->split.cnt) {  // forced: always the classic form
    *form = 1;
    return MI_RTJ_OK;
  }
  uint32_t w[4];
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(w, p->split.cnt, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *form = split == 1 ? 0 : split == 0 ? 1 : (int)w[2];
  *classic_launches_left = split < 0 ? (int)w[3] : 0;
  *parts_listed = (long long)w[p->split.flip ^ 1];  // the counter of the launch queued last (the next launch's is zero)
  return MI_RTJ_OK;
}

int mi_rtj_plan_spec_stats(mi_rtj_plan* p, int* proven, long long* walkers, long long* repaired) {
  if (!p || !proven || !walkers || !repaired) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = p->ctx;
  *proven = 0;
  *repaired = 0;
  *walkers = p->spec.on ? (long long)p->spec.n : 0;
  if (!p->spec.on) return MI_RTJ_OK;
  std::vector<uint32_t> ok(p->n);
  HIPCHK(c, hipSetDevice(c->device));
  uint32_t nfix = 0;
  HIPCHK(c, hipMemcpyAsync(ok.data(), p->spec.ok, sizeof(uint32_t) * p->n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&nfix, p->spec.nfix, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  uint32_t st[kSpecStWords] = {};
  if (p->spec.state) HIPCHK(c, hipMemcpyAsync(st, p->spec.state, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // (while the speculation is paused no walker runs and nobody zeroes the repair count: it is the last unpaused launch's)
  *repaired = st[kSpecStPause] ? 0 : nfix;
  for (uint32_t v : ok) *proven += v == 1u ? 1 : 0;
  return MI_RTJ_OK;
}

#ifdef MIRTJ_EXPERIMENTS
// timing builds only (not declared in include/mi_rtjpeg.h): ticks per section of the pooling chroma waves since the last call
extern "C" int mi_rtj_debug_pool_stamps(unsigned long long out[16]) {
  if (hipDeviceSynchronize() != hipSuccess) return MI_RTJ_ERR_HIP;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pool_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return MI_RTJ_ERR_HIP;
  unsigned long long zero[16] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_pool_stamps), zero, sizeof zero) != hipSuccess) return MI_RTJ_ERR_HIP;
  return MI_RTJ_OK;
}
#endif

int mi_rtj_plan_read_index(mi_rtj_plan* p, uint32_t* dst, size_t max_entries) {
  if (!p || !dst) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = p->ctx;
  std::vector<uint32_t> all(p->n_index);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (k_decode of the last launch waited for its index)
  HIPCHK(c, hipMemcpyAsync(all.data(), p->ov.last ? p->ov.blkoff_b.p : p->blkoff.p, sizeof(uint32_t) * p->n_index,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  size_t k = 0;
  for (int i = 0; i < p->n; i++) {
    const FrameDev& f = p->h_frames[i];
    const size_t cnt = (size_t)frame_blocks(f, p->fmt) + 1;
    if (k + cnt > max_entries) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_plan_read_index: destination too small");
    memcpy(dst + k, all.data() + f.blk_base, cnt * sizeof(uint32_t));
    k += cnt;
  }
  return MI_RTJ_OK;
}

// mi_rtj_plan_set_runs and mi_rtj_plan_set_runs_fmt behind their argument checks; `who` names the entry point in messages.
// The rows of the mask and carry arrays and the extent of an output picture are the plan's format's.
static int plan_set_runs(mi_rtj_plan* p, int n_runs, const int* run_len, const char* who) {
  mi_rtj_ctx* c = p->ctx;
  const Format& F = kFormats[p->fmt];
  if (n_runs < 0 || (n_runs > 0 && !run_len)) return fail(c, MI_RTJ_ERR_ARG, "%s: bad argument", who);
  // ---- check everything before anything changes: a refused call leaves the plan as it was ----
  std::vector<RunDev> runs;
  std::vector<RunChunkDev> chunks;
  uint64_t rows = 0, sum = 0;
  uint32_t nmb_max = 0;
  for (int r = 0; r < n_runs; r++) {
    if (run_len[r] <= 0) return fail(c, MI_RTJ_ERR_ARG, "%s: run %d has length %d", who, r, run_len[r]);
    sum += (uint64_t)run_len[r];
    if (sum > (uint64_t)p->n) break;
    const uint32_t f0 = (uint32_t)(sum - run_len[r]), len = (uint32_t)run_len[r];
    const FrameDev& a = p->h_frames[f0];
    std::vector<std::pair<uint64_t, uint64_t>> span;  // output pictures of the run
    for (uint32_t k = 0; k < len; k++) {
      const FrameDev& f = p->h_frames[f0 + k];
      if (f.w != a.w || f.h != a.h)
        return fail(c, MI_RTJ_ERR_ARG, "%s: packet %u of run %d is %ux%u, the run's picture 0 is %ux%u "
                    "(a size change inside a run is refused)", who, f0 + k, r, f.w, f.h, a.w, a.h);
      span.emplace_back(f.out_off, f.out_off + (uint64_t)F.picture_bytes(f.w, f.h));
    }
    std::sort(span.begin(), span.end());
    for (size_t k = 1; k < span.size(); k++)
      if (span[k].first < span[k - 1].second)
        return fail(c, MI_RTJ_ERR_ARG, "%s: output pictures of run %d overlap", who, r);
    if (len < 2) continue;  // picture 0 alone: nothing to resolve
    RunDev rd{};
    rd.chunk0 = (uint32_t)chunks.size();
    rd.nmb = a.nmb;
    for (uint32_t j = 0; j < len; j += kRunChunk) {
      RunChunkDev ch{};
      ch.frame0 = f0;
      ch.rel0 = j;
      ch.count = std::min<uint32_t>(kRunChunk, len - j);
      ch.nmb = a.nmb;
      ch.row = rows;
      rows += (uint64_t)F.blk_per_mb * a.nmb;
      chunks.push_back(ch);
    }
    rd.nchunks = (uint32_t)chunks.size() - rd.chunk0;
    runs.push_back(rd);
    nmb_max = std::max(nmb_max, a.nmb);
  }
  if (n_runs > 0 && sum != (uint64_t)p->n)
    return fail(c, MI_RTJ_ERR_ARG, "%s: run lengths add up to %llu, the plan has %d packets", who,
                (unsigned long long)sum, p->n);
  if ((uint64_t)chunks.size() * kRunSubs > 0xFFFFFFFFull)
    return fail(c, MI_RTJ_ERR_ARG, "%s: too many chunks", who);
  // ---- make the new state, then swap it in (launches queued before keep using the old one until they are done) ----
  HIPCHK(c, hipSetDevice(c->device));
  Runs q;
  q.n_runs = n_runs;
  q.list = (uint32_t)runs.size();
  q.chunks = (uint32_t)chunks.size();
  q.nmb_max = nmb_max;
  if (!chunks.empty()) {
    hipStream_t const s = c->stream;
    bool ok = q.d_runs.grow(c, runs.size(), s) == MI_RTJ_OK && q.d_chunks.grow(c, chunks.size(), s) == MI_RTJ_OK &&
              q.d_mask.grow(c, rows, s) == MI_RTJ_OK && q.d_carry.grow(c, rows, s) == MI_RTJ_OK &&
              q.d_copied.grow(c, 1, s, 0, true) == MI_RTJ_OK;
    hipError_t e = hipSuccess;
    if (ok) e = hipMemcpyAsync(q.d_runs, runs.data(), sizeof(RunDev) * runs.size(), hipMemcpyHostToDevice, s);
    if (ok && e == hipSuccess) e = hipMemcpyAsync(q.d_chunks, chunks.data(), sizeof(RunChunkDev) * chunks.size(), hipMemcpyHostToDevice, s);
    if (ok && e == hipSuccess) e = hipStreamSynchronize(s);  // (the host vectors go out of scope)
    if (!ok || e != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, MI_RTJ_ERR_NOMEM, "%s: %s (%llu chunk rows of %d runs)", who,
                  ok ? hipGetErrorString(e) : "out of device memory", (unsigned long long)chunks.size(), (int)runs.size());
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the old buffers may still be read by launches in flight
  p->runs = std::move(q);
  p->runs_ran = false;
  return MI_RTJ_OK;
}

int mi_rtj_plan_set_runs(mi_rtj_plan* p, int n_runs, const int* run_len) {
  if (!p) return MI_RTJ_ERR_ARG;
  if (n_runs < 0 || (n_runs > 0 && !run_len)) return fail(p->ctx, MI_RTJ_ERR_ARG, "mi_rtj_plan_set_runs: bad argument");
  if (p->fmt != MI_RTJ_FMT_YUV420)
    return fail(p->ctx, MI_RTJ_ERR_ARG, "mi_rtj_plan_set_runs: runs are for 4:2:0 plans; this plan's format is %s",
                kFormats[p->fmt].name);  // (mi_rtj_plan_set_runs_fmt takes plans of every format)
  return plan_set_runs(p, n_runs, run_len, "mi_rtj_plan_set_runs");
}

int mi_rtj_plan_set_runs_fmt(mi_rtj_plan* p, int n_runs, const int* run_len) {
  if (!p) return MI_RTJ_ERR_ARG;
  return plan_set_runs(p, n_runs, run_len, "mi_rtj_plan_set_runs_fmt");
}

int mi_rtj_plan_run_times(mi_rtj_plan* p, float* ms, int* launches) {
  if (!p || !ms) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = p->ctx;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *ms = 0.f;
  int n = 0;
  for (auto& t : p->run_ev) {
    if (!t.b) continue;
    float x = 0;
    HIPCHK(c, hipEventElapsedTime(&x, t.a, t.b));
    *ms += x;
    n++;
  }
  if (launches) *launches = n;
  return MI_RTJ_OK;
}

int mi_rtj_plan_run_stats(mi_rtj_plan* p, long long* copied) {
  if (!p || !copied) return MI_RTJ_ERR_ARG;
  mi_rtj_ctx* c = p->ctx;
  *copied = 0;
  if (!p->runs_ran) return MI_RTJ_OK;
  unsigned long long v = 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(&v, p->runs.d_copied, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *copied = (long long)v;
  return MI_RTJ_OK;
}

}  // extern "C" (reopened below)

namespace {
// Shared front half of the one-packet paths: header, (re)allocation, upload, the four kernels.
// On return the picture is being produced on c->stream into c->d_frame.
int decode_one_launch(mi_rtj_ctx* c, const uint8_t* pkt, size_t len) {
  if (!c || !pkt) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_decode: NULL argument");
  if (len < MI_RTJ_HEADER_SIZE) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_decode: packet shorter than its %d-byte header", MI_RTJ_HEADER_SIZE);
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->single) c->single = plan_new(c, 1, kPlanOnePacket);  // (its switches are read once per decoder, not once per packet)
  mi_rtj_plan* p = c->single;
  p->fmt = c->fmt;
  int rc = fill_frame(c, pkt, 0, (uint32_t)len, 0, 0, &p->h_frames[0]);
  if (rc != MI_RTJ_OK) return rc;
  c->fmt_fixed = true;
  const FrameDev& f = p->h_frames[0];
  // gavl_video_frame_create in init_rtjpeg (lib/video_rtjpeg.c:54): a larger picture starts from zeros
  if ((rc = c->d_frame.grow(c, frame_plane_bytes(f, p->fmt), c->stream, kAllocPad, true)) != MI_RTJ_OK) return rc;
  if (len + kAllocPad > c->d_pkt.cap && (rc = c->d_pkt.grow(c, (len + kAllocPad) * 2, c->stream)) != MI_RTJ_OK) return rc;
  if ((rc = plan_fit_index(p, frame_index_entries(f, p->fmt), 0)) != MI_RTJ_OK) return rc;
  p->n_blocks = frame_blocks(f, p->fmt);
  p->max_groups = frame_groups(f, p->fmt);
  // lays the packet's chunks out; allocates only when it is larger than any before it
  if (p->fmt == MI_RTJ_FMT_YUV420 && (rc = plan_alloc_chunks(p)) != MI_RTJ_OK) return rc;
  // pageable source: the runtime stages it; a private pinned staging copy measured no faster
  HIPCHK(c, hipMemcpyAsync(c->d_pkt, pkt, len, hipMemcpyHostToDevice, c->stream));
  if ((rc = plan_upload(p)) != MI_RTJ_OK) return rc;
  return plan_launch(p, c->d_pkt, c->d_frame);
}
}  // namespace

extern "C" {

int mi_rtj_decode(mi_rtj_ctx* c, const uint8_t* pkt, size_t len, uint8_t* const dst[3], const int dst_stride[3],
                  int crop_w, int crop_h) {
  const int r = decode_one_launch(c, pkt, len);
  if (r != MI_RTJ_OK) return r;
  const FrameDev& f = c->single->h_frames[0];
  if (dst) {
    // gavl_video_frame_copy(format, f, priv->frame) (lib/video_rtjpeg.c:82): image_width x
    // image_height region, each side's own strides — done by the copy engine on the way out.
    const Format& F = kFormats[c->fmt];
    const bool grey = F.chroma_planes == 0;  // one plane: dst[1], dst[2] and their strides are not looked at
    if (!dst[0] || (!grey && (!dst[1] || !dst[2])) || !dst_stride) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_decode: NULL plane");
    if (crop_w <= 0 || crop_h <= 0 || crop_w > (int)f.w || crop_h > (int)f.h)
      return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_decode: crop %dx%d outside the coded %ux%u picture", crop_w, crop_h, f.w, f.h);
    const size_t ysz = (size_t)f.w * f.h, csz = F.chroma_plane_bytes(f.w, f.h), cstride = f.w >> F.chroma_sx;
    // chroma: half the width; half the height too in 4:2:0, every line in 4:2:2 (a cropped odd size rounds up)
    const int cw = (crop_w + (1 << F.chroma_sx) - 1) >> F.chroma_sx, ch = (crop_h + (1 << F.chroma_sy) - 1) >> F.chroma_sy;
    HIPCHK(c, hipMemcpy2DAsync(dst[0], (size_t)dst_stride[0], c->d_frame, f.w, (size_t)crop_w, (size_t)crop_h, hipMemcpyDeviceToHost, c->stream));
    if (!grey) {
      HIPCHK(c, hipMemcpy2DAsync(dst[1], (size_t)dst_stride[1], c->d_frame + ysz, cstride, (size_t)cw, (size_t)ch, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpy2DAsync(dst[2], (size_t)dst_stride[2], c->d_frame + ysz + csz, cstride, (size_t)cw, (size_t)ch, hipMemcpyDeviceToHost, c->stream));
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MI_RTJ_OK;
}

int mi_rtj_decode_nocopy(mi_rtj_ctx* c, const uint8_t* pkt, size_t len, const uint8_t* planes[3], int strides[3]) {
  if (!planes || !strides) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_decode_nocopy: NULL argument");
  const int r = decode_one_launch(c, pkt, len);
  if (r != MI_RTJ_OK) return r;
  const FrameDev& f = c->single->h_frames[0];
  const Format& F = kFormats[c->fmt];
  const size_t ysz = (size_t)f.w * f.h, fsz = frame_plane_bytes(f, c->fmt);
  const int rc = c->h_frame.grow(c, fsz, nullptr);
  if (rc != MI_RTJ_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_frame, c->d_frame, fsz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  planes[0] = c->h_frame;
  strides[0] = (int)f.w;
  if (F.chroma_planes == 0) {
    planes[1] = planes[2] = nullptr;
    strides[1] = strides[2] = 0;
    return MI_RTJ_OK;
  }
  planes[1] = c->h_frame + ysz;
  planes[2] = planes[1] + F.chroma_plane_bytes(f.w, f.h);
  strides[1] = strides[2] = (int)(f.w >> F.chroma_sx);
  return MI_RTJ_OK;
}

}  // extern "C"

#include "rtj_host_pipe.h"
#include "rtj_host_encode.h"
