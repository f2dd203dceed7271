// The "8-phase" main loop of the 256 x 256 x 64 tile kernels (cdna_hip_programming.md, the 256^2 8-phase template): the ONE definition
// of the schedule.  gemm_bf16_8ph_kernel (gemm_bf16.hip), conv2_dinput8_kernel (conv2_dinput.hip) and t8_tile (gemm_tn8_bf16.hip)
// instantiate it; a wait count or a barrier is changed here and nowhere else (tests/test_cabi_cpu.py keeps copies out).
//
// For GEMMs with enough 256 x 256 tiles to fill the chip (ECAPA's 1 x 1 convolutions: M = 76 800, N, K = 1024 .. 3072; the
// training step's M = 10 240 layers).  The 128 x 128 kernel of gemm_bf16.hip is a lock-step structure (every wave: wait, barrier,
// fragments, MFMAs) and stops at ~36 % of the MFMA peak.  Here:
//   * 8 waves = 2 (M) x 4 (N), a wave owns 128 x 64 of the tile (32 accumulator tiles); the two wave rows run HALF A PHASE APART
//     (one extra barrier for wave row 1 at the start, one for wave row 0 at the end), so while one wave of a SIMD runs its 16
//     MFMAs the other one issues its LDS reads and its share of the next K-tile's loads;
//   * a K-tile is four phases, one 64 x 32 quadrant of the wave's tile each: (A rows 0-63 | B cols 0-31), (same A | B 32-63),
//     (A 64-127 | same B), (same A | B 0-31 again): 8 + 4, 4, 8, 4 fragment reads, 16 MFMAs per phase;
//   * operands go HBM/L2 -> LDS by global_load_lds_dwordx4 in 16 KiB units of 128 rows (A: the rows of one quadrant row of both
//     wave rows; B: the columns of one quadrant column of all four wave columns), one unit of the NEXT K-tile per phase, into the
//     other of two 64 KiB buffers; one counted s_waitcnt vmcnt(4) per phase (two units = 4 loads of this wave stay in flight),
//     never 0 inside the loop; a unit is read one phase after the wait + barrier that retire it and restaged >= 2 phases after
//     its last read;
//   * LDS rows of 128 bytes, 16-byte chunks XOR-swizzled by (row & 7) on the SOURCE address and on the read (the NT layout below;
//     the TN kernel keeps its operands row-major in 256-byte rows and transpose-reads them, see gemm_tn8_bf16.hip).
//
// A kernel supplies, under these names in the scope where it expands MA_G8_MAINLOOP (always_inline lambdas; U, I, J arrive as
// std::integral_constant values C0 .. C3):
//   stage(U, kt, buf)   this wave's two global_load_lds of unit U (0 = A q0, 1 = B q0, 2 = B q1, 3 = A q1: the order in which a
//                       K-tile first needs them) of K-tile kt into buffer buf - exactly two loads, the wait counts depend on it;
//   load_a(unit), load_b(unit)   the fragment reads of one quadrant row / column from the unit at that LDS address;
//   mma(I, J)           the 16 MFMAs of quadrant (I, J);
// beside `smem` (the two buffers), `nk` (K-tiles, >= 1) and `wr` (the wave row, wave >> 2), and two optional statements (they may
// use the loop's `kt`): NEXT_TILE runs in front of the first phase of a K-tile that has a successor to stage, PRE_MMA0 / PRE_MMA2 run
// in front of the MFMAs of phases 0 and 2, right after the A fragments of quadrant row 0 / 1 arrive.  The order in a kernel is
// MA_G8_STAGE_FIRST(); g8_start(wr); MA_G8_MAINLOOP(...); g8_finish(wr); what a kernel puts between them is outside the schedule
// (the phase stamps of the timeline build).
//
// Why macros: whatever calls the kernel's lambdas has to expand in the kernel's own body.  As __forceinline__ function templates the
// same statements are simplified once on their own, before they are inlined, and the device code changes (measured on this
// schedule: 811 of 5 876 assembly lines of conv2_dinput.hip for the four stage calls alone, 792 of 3 883 of gemm_tn8_bf16.hip for the
// loop); a macro expands to the tokens the three kernels had, and their assembly is the parent's.
#pragma once
#include "device_common.h"

namespace ma {

constexpr int k8Threads = 512, k8Unit = 128 * 128, k8Buf = 4 * k8Unit;  // units of a buffer: A q0 | B q0 | B q1 | A q1; two buffers

using C0 = std::integral_constant<int, 0>;
using C1 = std::integral_constant<int, 1>;
using C2 = std::integral_constant<int, 2>;
using C3 = std::integral_constant<int, 3>;

// K-tile 0 has been staged into buffer 0: wait for it; from here to g8_finish wave row 1 runs half a phase behind wave row 0
__device__ __forceinline__ void g8_start(int wr) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr == 1) __builtin_amdgcn_s_barrier();
}
__device__ __forceinline__ void g8_finish(int wr) {
  if (wr == 0) __builtin_amdgcn_s_barrier();  // (the barrier wave row 1 took at the start)
}

// ---- the NT layout (A and B both K-contiguous: the GEMM and the conv2 input gradient) -------------------------------------------------
// A unit is 128 rows of 128 bytes, 16-byte chunk c of row r at chunk slot c ^ (r & 7).  Lane (frow = lane & 15, fk = lane >> 4) reads
// unit row 64 wr + 16 i + frow of an A unit, 32 wc + 16 j + frow of a B unit, logical chunk 4 kk + fk: byte offset off_a / off_b for
// fragment 0, kk = 0; + 2048 per fragment (16 rows), kk = 1: ^ 64.
template <int N>
__device__ __forceinline__ void g8_nt_load(bf16x8 (&f)[N][2], const char* unit, int off) {  // f[fragment][kk]
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) f[i][kk] = *reinterpret_cast<const bf16x8*>(unit + ((off + i * 2048) ^ (kk << 6)));
}
template <int I, int J>  // quadrant (I, J): acc[4 I + i][2 J + j]
__device__ __forceinline__ void g8_nt_mma(f32x4 (&acc)[8][4], const bf16x8 (&af)[4][2], const bf16x8 (&bfr)[2][2]) {
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[4 * I + i][2 * J + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j][kk], af[i][kk], acc[4 * I + i][2 * J + j], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
}

}  // namespace ma

// The NT-layout state of a wave, declared in the kernel's scope from its `lane`, `wr`, `wc`: the fragment offsets, the zeroed
// accumulators acc[8][4], the fragments and the load_a / load_b / mma that MA_G8_MAINLOOP calls.  (A macro for the reason above: the
// offsets and the zeroing behind a function call change the device code of both kernels.)
#define MA_G8_NT_WAVE()                                                                                                    \
  const int frow = lane & 15, fk = lane >> 4;                                                                              \
  const int off_a = (wr * 64 + frow) * 128 + ((fk ^ (frow & 7)) << 4);                                                     \
  const int off_b = (wc * 32 + frow) * 128 + ((fk ^ (frow & 7)) << 4);                                                     \
  f32x4 acc[8][4];                                                                                                         \
  _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                                            \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};                                   \
  bf16x8 af[4][2], bfr[2][2]; /* [fragment][kk] */                                                                         \
  auto load_a = [&](const char* unit) __attribute__((always_inline)) { g8_nt_load(af, unit, off_a); };                     \
  auto load_b = [&](const char* unit) __attribute__((always_inline)) { g8_nt_load(bfr, unit, off_b); };                    \
  auto mma = [&](auto ic, auto jc) __attribute__((always_inline)) {                                                        \
    g8_nt_mma<decltype(ic)::value, decltype(jc)::value>(acc, af, bfr);                                                     \
  }

#define MA_G8_STAGE_FIRST() \
  stage(C0{}, 0, 0);        \
  stage(C1{}, 0, 0);        \
  stage(C2{}, 0, 0);        \
  stage(C3{}, 0, 0)
// One phase: fragment reads of this quadrant, one unit of the next K-tile, the counted wait, barrier, 16 MFMAs, barrier.
// MORE: another K-tile follows (nothing is staged under the last one, and its waits drain).
#define MA_G8_PHASE(MORE, READS, U, I, J, PRE_MMA)                                    \
  {                                                                                   \
    READS;                                                                            \
    if constexpr (MORE) stage(U{}, kt + 1, nb);                                       \
    __builtin_amdgcn_sched_barrier(0);                                                \
    if constexpr (MORE) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");              \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             \
    __builtin_amdgcn_s_barrier();                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                \
    PRE_MMA;                                                                          \
    mma(I{}, J{});                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                \
    __builtin_amdgcn_s_barrier();                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                \
  }
#define MA_G8_TILE(MORE, NEXT_TILE, PRE_MMA0, PRE_MMA2)                               \
  {                                                                                   \
    const char* cb = smem + (kt & 1) * k8Buf;                                         \
    const int nb = (kt + 1) & 1;                                                      \
    if constexpr (MORE) { NEXT_TILE; }                                                \
    MA_G8_PHASE(MORE, load_a(cb); load_b(cb + k8Unit), C0, C0, C0, PRE_MMA0)          \
    MA_G8_PHASE(MORE, load_b(cb + 2 * k8Unit), C1, C0, C1, )                          \
    MA_G8_PHASE(MORE, load_a(cb + 3 * k8Unit), C2, C1, C1, PRE_MMA2)                  \
    MA_G8_PHASE(MORE, load_b(cb + k8Unit), C3, C1, C0, )                              \
  }
#define MA_G8_MAINLOOP(NEXT_TILE, PRE_MMA0, PRE_MMA2)                                 \
  {                                                                                   \
    int kt = 0;                                                                       \
    for (; kt + 1 < nk; ++kt) MA_G8_TILE(true, NEXT_TILE, PRE_MMA0, PRE_MMA2)         \
    MA_G8_TILE(false, NEXT_TILE, PRE_MMA0, PRE_MMA2) /* the last K-tile: nothing left to stage */ \
  }
