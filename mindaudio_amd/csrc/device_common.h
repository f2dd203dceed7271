// Device helpers shared by every kernel file: the vector / address-space typedefs, the compile-time loop, the bf16 conversions, the
// wave reductions and the phase-stamp macro.  A kernel file includes this header and defines none of these again
// (tests/test_cabi_cpu.py checks it).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace ma {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void gl_void_t;
typedef __attribute__((address_space(1))) const void gl_cvoid_t;

template <int... Is, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>{}), ...);
}
// compile-time loop: every index inside f is a constant expression, so register arrays never need dynamic indexing
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

// ---- bf16 <-> f32 ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// (the bf16 sits in the low half of a 32-bit word whose high half is zero)
__device__ __forceinline__ float bf2f_lo(uint32_t h) { return __uint_as_float(h << 16); }
// round to nearest even; a NaN stays a (quiet) NaN
__device__ __forceinline__ uint16_t f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// round to bf16 and back (round to nearest even; what a bf16 store followed by a load does).  Separate from bf2f(f2bf(f)) on
// purpose: a NaN comes back UNCHANGED (payload and sign), not quieted through | 0x40 - the training epilogues hand the float on, and
// a NaN that reaches them must stay the NaN it was.
__device__ __forceinline__ float bf16_round(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return f;
  u += 0x7fffu + ((u >> 16) & 1u);
  return __uint_as_float(u & 0xffff0000u);
}

// Two f32 -> packed bf16x2 (lo in the low half), round to nearest even, in two forms.  Both emit the same single instruction
// (v_cvt_pk_bf16_f32), but the code AROUND it differs: the inline asm is opaque to the scheduler, and swapping one form for the other
// changed a quarter to a half of the instructions of every file it was tried on.  So the two are different helpers: a file keeps the
// form it has and does not switch without a measurement.
__device__ __forceinline__ uint32_t pack2_bf16(float lo, float hi) {
  const bf16x2 r = __builtin_convertvector((f32x2){lo, hi}, bf16x2);
  return *reinterpret_cast<const uint32_t*>(&r);
}
__device__ __forceinline__ uint32_t pack2_bf16_asm(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
// bf16_round of a pair through the hardware conversion: one v_cvt_pk_bf16_f32 + a shift and a mask instead of two five-instruction
// integer sequences (same round-to-nearest-even; NaNs come back as the conversion's quiet NaN)
__device__ __forceinline__ void bf16_round2(float& a, float& b) {
  const uint32_t pk = pack2_bf16(a, b);
  a = __uint_as_float(pk << 16);
  b = __uint_as_float(pk & 0xffff0000u);
}

// ---- reductions over the 64 lanes of a wave (every lane gets the result) ----------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_minmax(float v, bool is_max) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, 64);
    v = is_max ? fmaxf(v, o) : fminf(v, o);
  }
  return v;
}

// Cross-lane sums without the LDS crossbar (ds_bpermute costs an LDS round trip, ~100 ns each, eight of them in a row per
// LayerNorm): lanes {c, c + 16, c + 32, c + 48} through gfx950's row swaps - with both operands a copy of x,
// v_permlane16_swap leaves (x[row 0], x[row 0], x[row 2], x[row 2]) and (x[row 1], x[row 1], x[row 3], x[row 3]), whose sum is
// x[l] + x[l ^ 16] in every lane (tools/ubench/permlane_test.hip); v_permlane32_swap does the same with the 32-lane halves.
// (asm: the builtin with two identical operands is folded to 2 x by this hipcc.)  Quads through DPP.
__device__ __forceinline__ float sum_xor16(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}
__device__ __forceinline__ float sum_xor32(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}
__device__ __forceinline__ float max_xor16(float x) {  // max(x[l], x[l ^ 16]), the same swap
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}
__device__ __forceinline__ float max_xor32(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}
__device__ __forceinline__ float sum_quad(float x) {  // x[l] + x[l ^ 1] + x[l ^ 2] + x[l ^ 3]
  x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1, 0xf, 0xf, true));
  x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x4E, 0xf, 0xf, true));
  return x;
}

// ---- scalar helpers -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int div_small(int m, int d, float inv) {  // floor(m / d) for 0 <= m < 2^24, inv = 1 / d
  int q = (int)((float)m * inv);
  if (q * d > m) --q;
  if ((q + 1) * d <= m) ++q;
  return q;
}
// (v_rcp_f32 instead of an IEEE division: 1 ulp, invisible after the bf16 rounding of every consumer)
__device__ __forceinline__ float sigmoid_fast(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }


// XCD-aware bijective tile order: consecutive workgroup ids go to different XCDs (bid % 8); each XCD gets a contiguous run of the
// ntiles tiles, so that tiles which share an operand panel find it in that XCD's L2.
__device__ __forceinline__ int xcd_tile_order(int bid, int ntiles) {
  const int q = ntiles / 8, r = ntiles % 8, xcd = bid % 8, idx = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
// granule swizzle of a 256-byte LDS row (8 granules of 32 bytes): rows r = a + 4h + 8g (a < 4) of one transpose-read must hit
// different banks
__device__ __forceinline__ int swz_row256(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }

}  // namespace ma

// Phase stamp of the kernels' timeline builds (each file's own -D...PROF): ts[k] = wall_clock64() (100 MHz) once the wave's scalar
// and LDS traffic has drained.  The stamps stay in SGPRs (a store inside a main loop would break its counted vmcnt waits); each file
// writes its `ts` out at a point where nothing is in flight.
#define MA_PHASE_STAMP(ts, k)                          \
  do {                                                 \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    (ts)[(k)] = wall_clock64();                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
  } while (0)
