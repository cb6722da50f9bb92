// dv_host_hold.h — the held calls: macroblocks flagged as errors keep the stream's last good pixels (DESIGN.md section
// 9.6).  Included by mi_dv.hip after dv_host_systems.h; not a kernel header.
#pragma once
#include <vector>

#include "dv_host_systems.h"

namespace {
// room for `desc` bytes of descriptors and `rows` mask / carry entries (they only grow; what is sized together is waited
// for once)
int hold_buffers(mi_dv_ctx* c, size_t desc, size_t rows) {
  mi_dv_ctx::Hold& h = c->hold;
  int rc = h.d_held.grow(c, (uint64_t)kHoldCounters * kHoldCounterStride, nullptr);
  if (rc != MI_DV_OK) return rc;
  if (!h.desc_done) HIPCHK(c, hipEventCreateWithFlags(&h.desc_done.p, hipEventDisableTiming));
  if (desc > h.d_desc.cap) {  // (the last of the two to grow)
    rc = release_together(c, c->stream, h.h_desc, h.d_desc);
    if (rc == MI_DV_OK) rc = h.h_desc.grow(c, desc, nullptr);
    if (rc == MI_DV_OK) rc = h.d_desc.grow(c, desc, nullptr);
    if (rc != MI_DV_OK) return rc;
  }
  if (rows > h.d_carry.cap) {
    rc = release_together(c, c->stream, h.d_mask, h.d_carry);
    if (rc != MI_DV_OK) return rc;
    if (h.d_mask.grow(c, rows, nullptr) != MI_DV_OK || h.d_carry.grow(c, rows, nullptr) != MI_DV_OK)
      return fail(c, MI_DV_ERR_NOMEM, "mi_dv_decode_batch_held: no device memory for %zu mask entries", rows);
  }
  return MI_DV_OK;
}

void hold_forget(mi_dv_ctx* c) {
  if (c) c->hold.kept = -1;
}

// phase 1 (k_dv_decode over all n frames), then phase 2 for the runs that have a source: every argument is checked
// before anything is launched
int decode_held(mi_dv_ctx* c, const Row& r, const char* who, const void* d_frames, int n, void* d_pics, int n_runs,
                const int* run_len, const void* d_prev, unsigned sta_mask) {
  if (sta_mask > 0xFFFFu) return fail(c, MI_DV_ERR_ARG, "%s: STA mask 0x%x: one bit per STA value, at most 0xFFFF", who, sta_mask);
  const BatchCheck k{c, who};
  int rc = k.count(d_frames && d_pics && n_runs >= 0, n, "frames");
  if (rc == MI_DV_OK) rc = k.aligned(d_frames, d_pics, d_prev, "4-byte, d_pics and d_prev 8-byte");
  if (rc != MI_DV_OK) return rc;
  if (n_runs == 0 || !run_len) {  // one run
    n_runs = 1;
    run_len = &n;
  }
  long long sum = 0;
  for (int i = 0; i < n_runs; i++) {
    if (run_len[i] <= 0) return fail(c, MI_DV_ERR_ARG, "%s: run %d has %d frames", who, i, run_len[i]);
    sum += run_len[i];
  }
  if (sum != n) return fail(c, MI_DV_ERR_ARG, "%s: the %d runs hold %lld frames, the batch %d", who, n_runs, sum, n);
  if (d_prev) rc = k.apart(d_prev, (size_t)n_runs * r.pic_bytes, "d_prev", d_pics, (size_t)n * r.pic_bytes, "d_pics");
  if (rc != MI_DV_OK) return rc;
  if (!c) return fail(c, MI_DV_ERR_ARG, "%s: NULL instance", who);
  if (!sta_mask) sta_mask = MI_DV_STA_ERRORS;
  HIPCHK(c, hipSetDevice(c->device));
  mi_dv_ctx::Hold& h = c->hold;
  // a run has a source when it has an earlier picture of its own or one of d_prev
  std::vector<HoldChunkDev> chunks;
  std::vector<HoldRunDev> runs;
  uint32_t frame0 = 0;
  for (int i = 0; i < n_runs; i++) {
    const uint32_t len = (uint32_t)run_len[i];
    if (len >= 2u || d_prev) {
      runs.push_back({(uint32_t)chunks.size(), (len + kHoldChunk - 1u) / kHoldChunk});
      for (uint32_t rel = 0; rel < len; rel += kHoldChunk)
        chunks.push_back({frame0, rel, len - rel < (uint32_t)kHoldChunk ? len - rel : (uint32_t)kHoldChunk, (uint32_t)i});
    }
    frame0 += len;
  }
  const size_t chunk_bytes = chunks.size() * sizeof(HoldChunkDev), run_bytes = runs.size() * sizeof(HoldRunDev);
  if (!chunks.empty()) {
    rc = hold_buffers(c, chunk_bytes + run_bytes, chunks.size() * (size_t)r.nmb);
    if (rc != MI_DV_OK) return rc;
  }
  rc = decode_run(c, r, d_frames, n, d_pics);
  if (rc != MI_DV_OK) return rc;
  h.counted = false;
  if (chunks.empty()) return MI_DV_OK;
  HIPCHK(c, hipEventSynchronize(h.desc_done));  // (the last upload has left the pinned buffer; at once if there was none)
  memcpy(h.h_desc, chunks.data(), chunk_bytes);
  memcpy(h.h_desc + chunk_bytes, runs.data(), run_bytes);
  HIPCHK(c, hipMemcpyAsync(h.d_desc, h.h_desc, chunk_bytes + run_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(h.desc_done, c->stream));
  const HoldChunkDev* d_chunks = (const HoldChunkDev*)h.d_desc.p;
  const HoldRunDev* d_runs = (const HoldRunDev*)(h.d_desc + chunk_bytes);
  const uint32_t nchunks = (uint32_t)chunks.size(), nruns = (uint32_t)runs.size(), nmb = (uint32_t)r.nmb;
  const unsigned gx = (nmb + kHoldScanThreads - 1) / kHoldScanThreads;
  rc = h.time.begin(c, c->stream);
  if (rc != MI_DV_OK) return rc;
  hipLaunchKernelGGL(k_dv_hold_mask, dim3((nmb + kHoldMaskMbs - 1u) / kHoldMaskMbs, nchunks < kHoldMaxGridY ? nchunks : kHoldMaxGridY), dim3(kHoldScanThreads), 0, c->stream,
                     (const uint8_t*)d_frames, (uint32_t)r.frame_bytes, nmb, d_chunks, nchunks, (uint32_t)sta_mask, h.d_mask.p);
  hipLaunchKernelGGL(k_dv_hold_carry, dim3(gx, nruns < kHoldMaxGridY ? nruns : kHoldMaxGridY), dim3(kHoldScanThreads), 0, c->stream,
                     d_runs, nruns, d_chunks, nmb, (const uint64_t*)h.d_mask.p, h.d_carry.p, h.d_held.p);
  r.hold_copy(c->stream, d_chunks, nchunks * (uint32_t)kHoldSubs, h.d_mask, h.d_carry, (uint8_t*)d_pics, (const uint8_t*)d_prev, h.d_held);
  HIPCHK(c, hipGetLastError());
  rc = h.time.end(c, c->stream);
  h.counted = rc == MI_DV_OK;
  return rc;
}

// the macroblocks the last held batch took from another picture; synchronises
int hold_count(mi_dv_ctx* c, long long* held) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  unsigned long long v = 0;
  if (c->hold.counted) {  // the partial counts (dv_hold_kernels.h: kHoldCounters)
    std::vector<unsigned long long> part((size_t)kHoldCounters * kHoldCounterStride);
    HIPCHK(c, hipMemcpyAsync(part.data(), c->hold.d_held, part.size() * sizeof part[0], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < kHoldCounters; i++) v += part[(size_t)i * kHoldCounterStride];
  }
  *held = (long long)v;
  return MI_DV_OK;
}

// one host frame of system r (NULL: `system` is none) with held macroblocks from the picture this call made last
int decode_one_held(mi_dv_ctx* c, const Row* r, int system, const uint8_t* frame, size_t len, uint8_t* const planes[3],
                    const int strides[3], unsigned sta_mask, int* held) {
  const char* who = "mi_dv_decode_frame_held";
  // a refused frame, and one that failed on the way, leave no picture behind: the next frame has no source
  int rc = !r ? fail(c, MI_DV_ERR_ARG, "%s: unknown system %d", who, system)
           : sta_mask > 0xFFFFu ? fail(c, MI_DV_ERR_ARG, "%s: STA mask 0x%x: one bit per STA value, at most 0xFFFF", who, sta_mask)
                                : check_one(c, *r, who, frame, len, planes, strides);
  if (rc != MI_DV_OK) {
    hold_forget(c);
    return rc;
  }
  mi_dv_ctx::Hold& h = c->hold;
  const int at = (int)(r - kSystems);
  const bool had = h.kept == at;
  hold_forget(c);  // (until this frame's picture is there; a picture of another system is no source for a later frame)
  HIPCHK(c, hipSetDevice(c->device));
  rc = one_frame_buffers(c, *r);
  for (DevBuf<uint8_t>& d : h.keep[at])
    if (rc == MI_DV_OK) rc = d.grow(c, (uint64_t)r->pic_bytes, nullptr);
  if (rc != MI_DV_OK) return rc;
  uint8_t* const last = h.keep[at][h.cur[at]];
  uint8_t* const now = h.keep[at][h.cur[at] ^ 1];
  HIPCHK(c, hipMemcpyAsync(c->d_frame, frame, (size_t)r->frame_bytes, hipMemcpyHostToDevice, c->stream));
  rc = decode_held(c, *r, who, c->d_frame, 1, now, 0, nullptr, had ? last : nullptr, sta_mask);
  if (rc != MI_DV_OK) return rc;
  rc = planes_out(c, *r, now, planes, strides);
  if (rc != MI_DV_OK) return rc;
  if (held) {
    long long v = 0;
    rc = hold_count(c, &v);
    if (rc != MI_DV_OK) return rc;
    *held = (int)v;
  }
  h.cur[at] ^= 1;
  h.kept = at;
  return MI_DV_OK;
}
}  // namespace
