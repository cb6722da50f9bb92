// The speculative walker's byte step (csrc/rtj_spec_kernels.h) with the macroblock phase in registers (15 vector
// instructions: q, rb and three compares / selects per byte) against the phase in a per-lane LDS table (12: the raw-byte
// count comes out of the current entry by an SDWA byte select, a block end selects the entry read from LDS at the start
// of the same step).  Both run over the same synthetic bytes, held in registers as the walker holds a tile, with 4 waves
// per SIMD on every CU (10 KB of LDS per wave of 64), and must leave the same start bits.  The question is whether three
// other waves per SIMD hide the ds_read_b32 of every step.  gfx950, wave64.
//   hipcc -O3 --offload-arch=gfx950 spec_phase_step.hip -o spec_phase_step && ./spec_phase_step [iters] [blocks]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// the step as it was: phase in q, rb
#define STEP_REG(NSEL)                                                                                            \
  asm("v_cmp_eq_i32_e32 vcc, %[kn64], %[tm]\n\t"                                                                   \
      "v_cmp_lt_i32_e64 %[ma], %[u], %[rb]\n\t"                                                                    \
      "v_addc_co_u32_e64 %[bits], %[mz], %[bits], %[bits], %[em]\n\t"                                              \
      "s_and_b64 vcc, vcc, %[em]\n\t"                                                                              \
      "v_sub_u32_sdwa %[tn], sext(%[wn]), %[k63] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" NSEL             \
      " src1_sel:DWORD\n\t"                                                                                       \
      "v_cndmask_b32_e64 %[wr], 1, 64, vcc\n\t"                                                                    \
      "v_cndmask_b32_e64 %[wt], %[wtm], %[wr], %[ma]\n\t"                                                          \
      "v_add_u32_e32 %[u], %[u], %[wt]\n\t"                                                                        \
      "v_cmp_lt_i32_e64 %[em], 63, %[u]\n\t"                                                                       \
      "v_max_i32_e32 %[wtn], 1, %[tn]\n\t"                                                                         \
      "s_nop 0\n\t"                                                                                                \
      "v_subb_co_u32_e64 %[q], vcc, %[q], 0, %[em]\n\t"                                                            \
      "v_cmp_lt_i32_e64 %[mx], %[q], 0\n\t"                                                                        \
      "v_cmp_lt_u32_e64 %[my], %[q], 2\n\t"                                                                        \
      "v_cndmask_b32_e64 %[u], %[u], 0, %[em]\n\t"                                                                 \
      "v_cndmask_b32_e64 %[q], %[q], 5, %[mx]\n\t"                                                                 \
      "v_cndmask_b32_e64 %[rb], %[lb], %[cb], %[my]"                                                               \
      : [u] "+v"(u), [q] "+v"(q), [rb] "+v"(rb), [em] "+s"(em), [bits] "+v"(bits_), [tn] "=&v"(tn_), [wtn] "=&v"(wtn_), \
        [wt] "=&v"(wt_), [wr] "=&v"(wr_), [ma] "=&s"(ma_), [mx] "=&s"(mx_), [my] "=&s"(my_), [mz] "=&s"(mz_)         \
      : [tm] "v"(tm_), [wtm] "v"(wtm_), [wn] "v"(wn_), [k63] "v"(k63), [kn64] "v"(kn64), [lb] "v"(lb), [cb] "v"(cb)  \
      : "vcc", "scc")

// the phase in an LDS table: cu = the current phase's entry (byte 0: rb, bits 16-31: the LDS address of the next
// phase's entry), pt = that address, ready for the read.  PAD: what stands between the compare that writes em and its
// first reader besides the v_max (the wait alone, or the wait and an s_nop).
#define STEP_LDS(NSEL, PAD)                                                                                       \
  asm("ds_read_b32 %[nx], %[pt]\n\t"                                                                               \
      "v_cmp_eq_i32_e32 vcc, %[kn64], %[tm]\n\t"                                                                   \
      "v_cmp_lt_i32_sdwa %[ma], %[u], %[cu] src0_sel:DWORD src1_sel:BYTE_0\n\t"                                    \
      "v_addc_co_u32_e64 %[bits], %[mz], %[bits], %[bits], %[em]\n\t"                                              \
      "s_and_b64 vcc, vcc, %[em]\n\t"                                                                              \
      "v_sub_u32_sdwa %[tn], sext(%[wn]), %[k63] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" NSEL             \
      " src1_sel:DWORD\n\t"                                                                                       \
      "v_cndmask_b32_e64 %[wr], 1, 64, vcc\n\t"                                                                    \
      "v_cndmask_b32_e64 %[wt], %[wtm], %[wr], %[ma]\n\t"                                                          \
      "v_add_u32_e32 %[u], %[u], %[wt]\n\t"                                                                        \
      "v_cmp_lt_i32_e64 %[em], 63, %[u]\n\t"                                                                       \
      "v_max_i32_e32 %[wtn], 1, %[tn]\n\t"                                                                         \
      "s_waitcnt lgkmcnt(0)\n\t" PAD                                                                               \
      "v_cndmask_b32_e64 %[u], %[u], 0, %[em]\n\t"                                                                 \
      "v_cndmask_b32_e64 %[cu], %[cu], %[nx], %[em]\n\t"                                                           \
      "v_lshrrev_b32_e32 %[pt], 16, %[cu]"                                                                         \
      : [u] "+v"(u), [cu] "+v"(cu), [pt] "+v"(pt), [em] "+s"(em), [bits] "+v"(bits_), [tn] "=&v"(tn_),             \
        [wtn] "=&v"(wtn_), [wt] "=&v"(wt_), [wr] "=&v"(wr_), [nx] "=&v"(nx_), [ma] "=&s"(ma_), [mz] "=&s"(mz_)     \
      : [tm] "v"(tm_), [wtm] "v"(wtm_), [wn] "v"(wn_), [k63] "v"(k63), [kn64] "v"(kn64)                            \
      : "vcc", "scc")

// no phase at all (lb8 == cb8): the floor of this design, 10 instructions
#define STEP_ONE(NSEL)                                                                                            \
  asm("v_cmp_eq_i32_e32 vcc, %[kn64], %[tm]\n\t"                                                                   \
      "v_cmp_lt_i32_e64 %[ma], %[u], %[rb]\n\t"                                                                    \
      "v_addc_co_u32_e64 %[bits], %[mz], %[bits], %[bits], %[em]\n\t"                                              \
      "s_and_b64 vcc, vcc, %[em]\n\t"                                                                              \
      "v_sub_u32_sdwa %[tn], sext(%[wn]), %[k63] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" NSEL             \
      " src1_sel:DWORD\n\t"                                                                                       \
      "v_cndmask_b32_e64 %[wr], 1, 64, vcc\n\t"                                                                    \
      "v_cndmask_b32_e64 %[wt], %[wtm], %[wr], %[ma]\n\t"                                                          \
      "v_add_u32_e32 %[u], %[u], %[wt]\n\t"                                                                        \
      "v_cmp_lt_i32_e64 %[em], 63, %[u]\n\t"                                                                       \
      "v_max_i32_e32 %[wtn], 1, %[tn]\n\t"                                                                         \
      "s_nop 0\n\t"                                                                                                \
      "v_cndmask_b32_e64 %[u], %[u], 0, %[em]"                                                                     \
      : [u] "+v"(u), [em] "+s"(em), [bits] "+v"(bits_), [tn] "=&v"(tn_), [wtn] "=&v"(wtn_), [wt] "=&v"(wt_),       \
        [wr] "=&v"(wr_), [ma] "=&s"(ma_), [mz] "=&s"(mz_)                                                          \
      : [tm] "v"(tm_), [wtm] "v"(wtm_), [wn] "v"(wn_), [k63] "v"(k63), [kn64] "v"(kn64), [rb] "v"(rb)              \
      : "vcc", "scc")

constexpr int kLdsPerWave = 10240;  // 16 waves of 64 per CU (160 KB): 4 per SIMD

// K: 0 the step as it was, 1 the table (wait only), 2 the table (wait + s_nop), 3 no phase
template <int K>
__global__ __launch_bounds__(64) void k_step(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int iters,
                                             int lb, int cb) {
  __shared__ __attribute__((aligned(16))) uint32_t s_mem[kLdsPerWave / 4];
  const int lane = threadIdx.x;
  const uint32_t g = blockIdx.x * 64u + (uint32_t)lane;
  uint32_t cur[33];
#pragma unroll
  for (int k = 0; k < 32; k++) cur[k] = in[(size_t)k * gridDim.x * 64u + g];
  cur[32] = cur[0];
  const uint32_t tab = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)s_mem;
  for (int p = 0; p < 6; p++)
    s_mem[p * 64 + lane] = ((tab + (uint32_t)(((p + 1) % 6) * 256 + lane * 4)) << 16) | ((uint32_t)p << 8) | (uint32_t)(p < 4 ? lb : cb);
  asm volatile("" ::"v"(tab) : "memory");  // the table is written before the steps read it (LDS keeps a wave's order)
  int u = 0, rb = lb;
  uint32_t q = 5, cu = s_mem[lane], pt = cu >> 16;
  uint64_t em = ~0ull;
  const int kn64 = -64, k63 = 63;
  uint32_t sum = 0;
  int tm_ = (int)(int8_t)(cur[0] & 0xFFu) - 63, wtm_ = tm_ > 1 ? tm_ : 1;
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t wd[5] = {cur[4 * i], cur[4 * i + 1], cur[4 * i + 2], cur[4 * i + 3], cur[4 * i + 4]};
      uint32_t bits_ = 0;
#pragma unroll
      for (int b = 0; b < 16; b++) {
        const uint32_t wn_ = wd[(b + 1) >> 2];
        int tn_, wtn_, wt_, wr_;
        uint32_t nx_;
        uint64_t ma_, mx_, my_, mz_;
#define ONE(NSEL)                                   \
  if (K == 0) STEP_REG(NSEL);                       \
  else if (K == 1) STEP_LDS(NSEL, "");              \
  else if (K == 2) STEP_LDS(NSEL, "s_nop 0\n\t");   \
  else STEP_ONE(NSEL)
        switch ((b + 1) & 3) {
          case 0: ONE("BYTE_0"); break;
          case 1: ONE("BYTE_1"); break;
          case 2: ONE("BYTE_2"); break;
          default: ONE("BYTE_3"); break;
        }
        tm_ = tn_;
        wtm_ = wtn_;
      }
      sum = sum * 0x9E3779B1u + bits_;
    }
  }
  const uint32_t phase = K == 0 ? 5u - q : K == 3 ? 0u : (cu >> 8) & 0xFFu;
  out[g] = sum ^ ((uint32_t)u << 8) ^ phase;
}

template <int K>
static float run(const uint32_t* d_in, uint32_t* d_out, int blocks, int iters, int lb, int cb) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  CK(hipEventRecord(a));
  hipLaunchKernelGGL(k_step<K>, dim3(blocks), dim3(64), 0, 0, d_in, d_out, iters, lb, cb);
  CK(hipEventRecord(b));
  CK(hipEventSynchronize(b));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, a, b));
  CK(hipEventDestroy(a));
  CK(hipEventDestroy(b));
  return ms;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 64;
  const int blocks = argc > 2 ? atoi(argv[2]) : 256 * 16 * 4;  // four generations of 16 waves per CU
  const int lb = 10, cb = 1;                                  // Q = 255: lb8 = 9, cb8 = 0
  const size_t lanes = (size_t)blocks * 64, n = lanes * 32;
  uint32_t* h = (uint32_t*)malloc(n * 4);
  // bytes as an encoder makes them, roughly: small tokens, now and then a long zero run (a block end), 0xFF one-byte
  // blocks alone and in runs
  uint64_t s = 0x2545F4914F6CDD1Dull;
  auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  for (size_t l = 0; l < lanes; l++) {
    int ff = 0;
    for (int k = 0; k < 32; k++) {
      uint32_t w = 0;
      for (int j = 0; j < 4; j++) {
        const uint32_t r = rnd();
        uint32_t byte = (r & 15u) == 0 ? 64u + ((r >> 8) & 63u) : (r >> 8) & 63u;
        if (ff == 0 && (r >> 16) % 61u == 0) ff = 1 + (int)((r >> 24) % 20u);
        if (ff > 0) { byte = 255u; ff--; }
        w |= byte << (8 * j);
      }
      h[(size_t)k * lanes + l] = w;
    }
  }
  uint32_t *d_in, *d_out;
  CK(hipMalloc(&d_in, n * 4));
  CK(hipMalloc(&d_out, lanes * 4 * 4));
  CK(hipMemcpy(d_in, h, n * 4, hipMemcpyHostToDevice));
  uint32_t* o = (uint32_t*)malloc(lanes * 4 * 4);
  const char* names[4] = {"registers, 15 instructions", "LDS table, 12 (wait)", "LDS table, 12 (wait + s_nop)", "no phase, 10"};
  float best[4] = {1e30f, 1e30f, 1e30f, 1e30f};
  for (int rep = 0; rep < 5; rep++) {  // alternating, the first round warms up
    const float t[4] = {run<0>(d_in, d_out, blocks, iters, lb, cb), run<1>(d_in, d_out + lanes, blocks, iters, lb, cb),
                        run<2>(d_in, d_out + 2 * lanes, blocks, iters, lb, cb), run<3>(d_in, d_out + 3 * lanes, blocks, iters, lb, cb)};
    printf("rep %d:", rep);
    for (int k = 0; k < 4; k++) {
      printf(" %.3f", t[k]);
      if (rep && t[k] < best[k]) best[k] = t[k];
    }
    printf(" ms\n");
  }
  CK(hipMemcpy(o, d_out, lanes * 4 * 4, hipMemcpyDeviceToHost));
  size_t bad1 = 0, bad2 = 0;
  for (size_t l = 0; l < lanes; l++) {
    bad1 += o[l] != o[lanes + l];
    bad2 += o[l] != o[2 * lanes + l];
  }
  const double steps = (double)iters * 128.0;
  // cycles a SIMD spends per byte step of one wave, at 2.4 GHz: waves per SIMD = blocks / 1024
  for (int k = 0; k < 4; k++)
    printf("%-30s %8.3f ms  %6.2f cycles per step and wave\n", names[k], best[k],
           best[k] * 1e-3 * 2.4e9 / (steps * (double)blocks / 1024.0));
  printf("lanes whose result differs from the register step's: %zu (wait), %zu (wait + s_nop) of %zu\n", bad1, bad2, lanes);
  return bad1 || bad2 ? 2 : 0;
}
