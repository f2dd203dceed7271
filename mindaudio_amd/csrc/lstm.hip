// Bidirectional LSTM layer, inference (mindaudio/models/deepspeech2.py BatchRNN: nn.LSTM(bidirectional=True, has_bias=True), the two
// directions SUMMED).  Contract: include/mindaudio_amd.h.  The tile, the cell, the packed weights' fragment order and the K loop are
// lstm_common.h's; this file holds the schedule, the direction sum and the two ways a workgroup covers its batch rows.
// The training forward (ma_lstm_bidir_train_bf16) is the same code under the compile-time flag TAPE: it also writes what the backward
// pass of lstm_train.hip reads.  The TAPE = false instantiations are the inference kernels, instruction for instruction.
//
// Schedule.  One layer = the input projection of a time chunk (ma_gemm_bf16, float32 out, b_ih + b_hh as its bias) followed by ONE
// LAUNCH PER TIME STEP of a step kernel, issued from the host loop of ma_lstm_bidir_bf16.  The stream order between those launches is
// the only synchronisation: no workgroup ever waits for another one (no grid barrier, no flags, no cooperative launch, no atomics).
//
// Step kernel.  gates (B, 4H) = h_{s-1} (B, H) . W_hh^T + the step's projection rows; c is float32, updated in place, one owner per
// element.  grid = (H / 16 hidden slices, directions, ceil(B / 64)), 4 waves per workgroup, wave w runs the cell of batch rows
// 64 z + 16 w .. + 15.  W_hh is packed once (ma_lstm_pack_f32) with the two directions as 2 H / 16 slices; h is read from its
// (B, H) bf16 image, 16 bytes per lane.  Two forms:
//   lstm_step_ksplit_kernel (H / 32 a multiple of 4): K is split over the four waves, each runs a quarter of the k-steps for all four
//     batch tiles, so the workgroup reads its 128 KB slice of W_hh once; the partial sums meet in LDS (48 KB, one workgroup barrier).
//   lstm_step_kernel (any H % 64 == 0): each wave runs all of K for its own tile; no LDS, no barrier.
//
// Rounding points: x, W_ih, W_hh and the fed-back h are bf16 MFMA operands (round to nearest even); the projection, the gate sums,
// c, h before it is fed back, and the layer output are float32; accumulation is float32.
//
// Direction sum: out[t] = h_fwd[t] + h_bwd[t].  Step s serves t = s (forward) and t = T - 1 - s (reverse).  The direction that reaches
// a t first stores its h into out_f32[t]; the one that reaches it later (a later launch) adds its own and stores the float32 sum and
// its bf16 rounding (the next GEMM's operand).  For odd T both meet at t = (T - 1) / 2 in ONE launch: the forward half goes to out_f32,
// the reverse half to a (B, H) side buffer and one pointwise launch joins them.  a + b == b + a in float32, so the order never shows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "launch.h"
#include "lstm_common.h"

namespace ma {

enum : int { kLstmFirst = 0, kLstmSecond = 1, kLstmAlone = 2, kLstmTie = 3 };

struct LstmStep {
  const float* proj[2];  // this step's (B, 4H) projection rows per direction
  const uint16_t* whh;   // packed, both directions
  const uint16_t* h_in;  // (2, B, H) bf16: h_{s-1}
  uint16_t* h_out;       // (2, B, H) bf16: h_s
  float* c;              // (2, B, H)
  float* out_f32[2];     // row block t of (T, B, H) per direction
  uint16_t* out_bf16[2];
  float* tie;            // (B, H)
  int32_t mode[2];
  int32_t dir0;          // direction of blockIdx.y == 0
  int32_t B, H;
};

// The training forward is the same step with a TAPE: the step's frame of the tape per direction (lstm_common.h: five (B, H) float32
// planes i, f, g, o, c, and the bf16 h image).  The inference step carries none of it: LstmStepT<false> is LstmStep.
template <bool TAPE>
struct LstmStepT : LstmStep {};
template <>
struct LstmStepT<true> : LstmStep {
  float* tape_act[2];     // (5, B, H) of frame t
  uint16_t* tape_h[2];    // (B, H) of frame t
};

// What the cell of one 16 x 16 tile reads besides the product, in the C/D layout (batch row b0 + 4 (lane >> 4) + r, hidden unit
// 16 sl + (lane & 15)): the four projections, c and - for the direction that reaches a frame second - the other direction's h.
// Rows beyond B read nothing.
struct LstmCellIn {
  float gate[4][4];  // [gate][r]
  float c[4], prev[4];
};
__device__ __forceinline__ LstmCellIn lstm_cell_load(const LstmStep& p, int dir, int sl, int b0, int lane) {
  const int H = p.H;
  const int64_t dir_off = (int64_t)dir * p.B * H;
  const int j = sl * kLstmSlice + (lane & 15);
  LstmCellIn in;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + 4 * (lane >> 4) + r;
    const bool ok = b < p.B;
    const float* pr = p.proj[dir] + (int64_t)(ok ? b : 0) * 4 * H + j;
    const int64_t e = (int64_t)(ok ? b : 0) * H + j;
#pragma unroll
    for (int g = 0; g < 4; ++g) in.gate[g][r] = ok ? pr[g * H] : 0.0f;
    in.c[r] = ok ? p.c[dir_off + e] : 0.0f;
    in.prev[r] = (ok && p.mode[dir] == kLstmSecond) ? p.out_f32[dir][e] : 0.0f;
  }
  return in;
}

// The gate sums, the cell and the stores of a tile.  Rows beyond B store nothing.
template <bool TAPE>
__device__ __forceinline__ void lstm_cell_store(const LstmStepT<TAPE>& p, int dir, int sl, int b0, int lane, const f32x4 (&acc)[4],
                                                const LstmCellIn& in) {
  const int H = p.H;
  const int64_t dir_off = (int64_t)dir * p.B * H;
  const int j = sl * kLstmSlice + (lane & 15);
  const int mode = p.mode[dir];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + 4 * (lane >> 4) + r;
    if (b >= p.B) continue;
    const int64_t e = (int64_t)b * H + j;
    const auto o = [&] {
      if constexpr (TAPE)
        return lstm_cell_taped(acc[0][r] + in.gate[0][r], acc[1][r] + in.gate[1][r], acc[2][r] + in.gate[2][r],
                               acc[3][r] + in.gate[3][r], in.c[r]);
      else
        return lstm_cell(acc[0][r] + in.gate[0][r], acc[1][r] + in.gate[1][r], acc[2][r] + in.gate[2][r], acc[3][r] + in.gate[3][r],
                         in.c[r]);
    }();
    p.c[dir_off + e] = o.c;
    p.h_out[dir_off + e] = f2bf(o.h);
    if constexpr (TAPE) {
      const int64_t plane = (int64_t)p.B * H;
      float* ta = p.tape_act[dir] + e;
      ta[0] = o.i;
      ta[plane] = o.f;
      ta[2 * plane] = o.g;
      ta[3 * plane] = o.o;
      ta[4 * plane] = o.c;
      p.tape_h[dir][e] = f2bf(o.h);
    }
    if (mode == kLstmFirst) {
      p.out_f32[dir][e] = o.h;
    } else if (mode == kLstmTie) {
      p.tie[e] = o.h;
    } else {
      const float v = mode == kLstmSecond ? in.prev[r] + o.h : o.h;
      p.out_f32[dir][e] = v;
      if (p.out_bf16[dir]) p.out_bf16[dir][e] = f2bf(v);
    }
  }
}

// this lane's A operand row of the tile at batch row b0 (rows beyond B take row 0's), at the lane's column of k-step 0
__device__ __forceinline__ const uint16_t* lstm_h_row(const LstmStep& p, int dir, int b0, int lane) {
  const int row = b0 + (lane & 15);
  return p.h_in + (int64_t)dir * p.B * p.H + (int64_t)(row < p.B ? row : 0) * p.H + 8 * (lane >> 4);
}

// Each wave runs all of K for its own batch tile (the form for an H / 32 that is no multiple of 4; launched with KB = 2).  KB =
// k-steps per operand block (5 KB of 16 bytes per lane).
template <int KB, bool TAPE>
__global__ __launch_bounds__(kLstmThreads) void lstm_step_kernel(const LstmStepT<TAPE> p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b0 = ((int)blockIdx.z * 4 + wave) * 16;
  if (b0 >= p.B) return;  // (no barrier anywhere in this kernel)
  const int dir = p.dir0 + (int)blockIdx.y, sl = blockIdx.x;
  const int nk = p.H / 32, ns = p.H / kLstmSlice;
  const uint16_t* hp = lstm_h_row(p, dir, b0, lane);
  f32x4 acc[1][4];
  LstmCellIn in;
  lstm_k_loop<KB>(lstm_gate_run(p.whh, nk, (int64_t)dir * ns + sl, 0, lane), [&](int, int kk) { return hp + kk * 32; }, 0, nk, acc,
                  [&] { in = lstm_cell_load(p, dir, sl, b0, lane); });
  lstm_cell_store(p, dir, sl, b0, lane, acc[0], in);
}

constexpr int kLstmPartialFloats = 4 * 3 * 16 * 64;  // [source wave][other tile][gate * 4 + register][lane]: 48 KB

// The same step with K SPLIT OVER THE FOUR WAVES (H / 32 a multiple of 4): wave w runs the k-steps [w nk / 4, (w + 1) nk / 4) for all
// four batch tiles of the workgroup, so the workgroup reads its 128 KB slice of W_hh once instead of once per wave.  The partial
// accumulators of the three tiles a wave does not own go through LDS; after the workgroup's one barrier wave w adds the four
// partials of tile w in wave order and runs the cell.  Tiles beyond B compute on row 0's operand and store nothing.
template <int KB, bool TAPE>
__global__ __launch_bounds__(kLstmThreads) void lstm_step_ksplit_kernel(const LstmStepT<TAPE> p) {
  __shared__ float part[kLstmPartialFloats];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int z0 = (int)blockIdx.z * kLstmRowsPerWg;
  const int dir = p.dir0 + (int)blockIdx.y, sl = blockIdx.x;
  const int nk = p.H / 32, ns = p.H / kLstmSlice, nkw = nk / 4;
  const uint16_t* hp[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) hp[t] = lstm_h_row(p, dir, z0 + 16 * t, lane) + wave * nkw * 32;  // (both operands start at the wave's share)
  const uint16_t* wp = lstm_gate_run(p.whh, nk, (int64_t)dir * ns + sl, wave * nkw, lane);
  f32x4 acc[4][4];  // [tile][gate]
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[t][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  // lstm_k_loop<KB, 4> written out: the same statements in the same order.  Through the call, with the cell's loads behind a callable,
  // this kernel's step measured 0.08 us longer at B = 1 (TasNet's layered schedule, 13 280 steps: 66.2 ms against 65.1 ms), so it
  // keeps the loop in its own body; a change to lstm_k_loop's issue order is made here as well.
  using Operands = LstmOperands<KB, 4>;
  auto load = [&](Operands& o, int kk0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < KB; ++u) {
#pragma unroll
      for (int g = 0; g < 4; ++g) o.w[u][g] = *reinterpret_cast<const bf16x8*>(wp + ((int64_t)(kk0 + u) * 4 + g) * kLstmGateElems);
#pragma unroll
      for (int t = 0; t < 4; ++t) o.a[u][t] = *reinterpret_cast<const bf16x8*>(hp[t] + (kk0 + u) * 32);
    }
  };
  auto mma = [&](const Operands& o) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < KB; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(o.a[u][t], o.w[u][g], acc[t][g], 0, 0, 0);
  };
  Operands cur, nxt;
  load(cur, 0);
  const LstmCellIn in = lstm_cell_load(p, dir, sl, z0 + 16 * wave, lane);
  for (int kk = KB; kk < nkw; kk += KB) {  // (nkw % KB == 0: the launcher's choice of KB)
    load(nxt, kk);
    mma(cur);
    cur = nxt;
  }
  mma(cur);

  // tile t's partial from wave s != t sits in slot (t - s - 1) & 3 (0 .. 2) of wave s's block
  f32x4 own[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t == wave) {
#pragma unroll
      for (int g = 0; g < 4; ++g) own[g] = acc[t][g];
    } else {
      float* dst = part + ((wave * 3 + ((t - wave - 1) & 3)) * 16) * 64 + lane;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(g * 4 + r) * 64] = acc[t][g][r];
    }
  }
  __syncthreads();  // (within the workgroup; every wave arrives: nothing returns before this line)
  f32x4 tot[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) tot[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {  // wave order = K order
    if (s == wave) {
#pragma unroll
      for (int g = 0; g < 4; ++g) tot[g] += own[g];
    } else {
      const float* src = part + ((s * 3 + ((wave - s - 1) & 3)) * 16) * 64 + lane;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) tot[g][r] += src[(g * 4 + r) * 64];
    }
  }
  lstm_cell_store(p, dir, sl, z0 + 16 * wave, lane, tot, in);
}

// the middle frame of an odd T: out = out (forward half) + tie (reverse half)
__global__ __launch_bounds__(256) void lstm_tie_kernel(float* __restrict__ out, uint16_t* __restrict__ out_bf, const float* __restrict__ tie,
                                                       int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = out[i] + tie[i];
  out[i] = v;
  if (out_bf) out_bf[i] = f2bf(v);
}

// W_ih (2, 4H, K) f32 -> (2, 4H, Kpad) bf16 with zero columns K .. Kpad - 1; bias = b_ih + b_hh
__global__ __launch_bounds__(256) void lstm_pack_ih_kernel(const float* __restrict__ w, const float* __restrict__ b_ih,
                                                           const float* __restrict__ b_hh, int K, int Kpad, int64_t rows,
                                                           uint16_t* __restrict__ out, float* __restrict__ bias) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < rows) bias[i] = b_ih[i] + b_hh[i];
  if (i >= rows * Kpad) return;
  const int64_t r = i / Kpad;
  const int k = (int)(i - r * Kpad);
  out[i] = k < K ? f2bf(w[r * K + k]) : (uint16_t)0;
}

// W_hh (2, 4H, H) f32 -> fragment order, the directions as 2 H / 16 slices
__global__ __launch_bounds__(256) void lstm_pack_hh_kernel(const float* __restrict__ w, int H, int64_t groups, uint16_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one 8-element fragment
  if (i >= groups) return;
  const LstmFragment f = lstm_fragment(i, H / 32);
  const int64_t dir = f.unit / H, j = f.unit % H;
  lstm_pack_fragment(w + ((dir * 4 + f.gate) * H + j) * H, f.k, H, out + i * 8);
}

struct LstmWs {
  int64_t h, c, tie, proj, total;  // byte offsets; proj holds 2 x (chunk * B, 4H) float32
};
static LstmWs lstm_ws(int64_t B, int64_t H, int64_t chunk) {
  LstmWs w;
  w.h = 0;
  w.c = w.h + align256(2 * 2 * B * H * 2);
  w.tie = w.c + align256(2 * B * H * 4);
  w.proj = w.tie + align256(B * H * 4);
  w.total = w.proj + 2 * align256(chunk * B * 4 * H * 4);
  return w;
}

}  // namespace ma

using namespace ma;

extern "C" {

int64_t ma_lstm_workspace_bytes(int64_t T, int64_t B, int32_t H, int64_t time_chunk) {
  if (T < 1 || B < 1 || H < 1 || time_chunk < 1) return MA_ERR_INVALID_ARG;
  if (!lstm_shape_ok(T, B, 64, H)) return MA_ERR_UNSUPPORTED;
  return lstm_ws(B, H, time_chunk < T ? time_chunk : T).total;
}

int ma_lstm_pack_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int32_t K, int32_t Kpad, int32_t H,
                     void* wih_bf16, void* whh_packed, float* bias, ma_stream_t stream) {
  if (!w_ih || !w_hh || !b_ih || !b_hh || !wih_bf16 || !whh_packed || !bias || K < 1 || Kpad < K || H < 1) return MA_ERR_INVALID_ARG;
  if (!lstm_shape_ok(1, 1, Kpad, H)) return MA_ERR_UNSUPPORTED;
  if (!lstm_aligned16(wih_bf16, whh_packed, bias)) return MA_ERR_INVALID_ARG;
  const int64_t rows = 2 * 4 * (int64_t)H, n_ih = rows * Kpad, groups = rows * H / 8;
  MA_LAUNCH(lstm_pack_ih_kernel, dim3((unsigned)((n_ih + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_ih, b_ih, b_hh, K, Kpad, rows,
            reinterpret_cast<uint16_t*>(wih_bf16), bias);
  MA_LAUNCH(lstm_pack_hh_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_hh, H, groups,
            reinterpret_cast<uint16_t*>(whh_packed));
  return MA_OK;
}

}  // extern "C"

namespace ma {

// The layer: ma_lstm_bidir_bf16 (TAPE = false) and ma_lstm_bidir_train_bf16 (TAPE = true: the same launches of the step kernels'
// taping instantiations, which also fill `tape`, lstm_common.h's layout).
template <bool TAPE>
static int lstm_bidir_run(const void* x, int64_t T, int64_t B, int32_t Kpad, int32_t H, const void* wih_bf16, const void* whh_packed,
                          const float* bias, int32_t dir_mask, int64_t time_chunk, float* out_f32, void* out_bf16, float* c_final,
                          void* tape, int64_t tape_bytes, void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  if (!x || !wih_bf16 || !whh_packed || !bias || !out_f32 || !workspace || (TAPE && !tape) || T < 1 || B < 1 || Kpad < 1 || H < 1 ||
      time_chunk < 1 || dir_mask < 1 || dir_mask > 3)
    return MA_ERR_INVALID_ARG;
  if (!lstm_shape_ok(T, B, Kpad, H)) return MA_ERR_UNSUPPORTED;
  if (!lstm_aligned16(x, wih_bf16, whh_packed, bias, workspace) || (TAPE && !lstm_aligned16(tape))) return MA_ERR_INVALID_ARG;
  const int64_t chunk = time_chunk < T ? time_chunk : T;
  const LstmWs ws = lstm_ws(B, H, chunk);
  if (workspace_bytes < ws.total) return MA_ERR_WORKSPACE;
  const LstmTapeLayout tl = lstm_tape_layout(T, B, H);
  if (TAPE && tape_bytes < tl.total) return MA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(workspace);
  uint16_t* hbuf = reinterpret_cast<uint16_t*>(base + ws.h);
  float* c = reinterpret_cast<float*>(base + ws.c);
  float* projbuf[2] = {reinterpret_cast<float*>(base + ws.proj),
                       reinterpret_cast<float*>(base + ws.proj + (ws.total - ws.proj) / 2)};
  const int64_t bh = B * H, g4 = 4 * (int64_t)H;
  if (ensure_init() != MA_OK) return MA_ERR_LAUNCH;
  // h_0 = c_0 = 0 (only the first of the two h images is read by step 0)
  if (hipMemsetAsync(hbuf, 0, (size_t)(2 * bh * 2), st) != hipSuccess) return MA_ERR_LAUNCH;
  if (hipMemsetAsync(c, 0, (size_t)(2 * bh * 4), st) != hipSuccess) return MA_ERR_LAUNCH;

  const uint16_t* xb = reinterpret_cast<const uint16_t*>(x);
  const uint16_t* wih = reinterpret_cast<const uint16_t*>(wih_bf16);
  uint16_t* obf = reinterpret_cast<uint16_t*>(out_bf16);
  const bool both = dir_mask == 3;
  const dim3 grid((unsigned)(H / kLstmSlice), both ? 2u : 1u, (unsigned)((B + kLstmRowsPerWg - 1) / kLstmRowsPerWg));

  ma_gemm_epilogue_t epi = ma_gemm_epilogue_t{};
  epi.alpha = 1.0f;
  for (int64_t s0 = 0; s0 < T; s0 += chunk) {
    const int64_t n = T - s0 < chunk ? T - s0 : chunk;
    const int64_t t0[2] = {s0, T - s0 - n};  // first frame of this chunk per direction (the reverse one walks it backwards)
    for (int d = 0; d < 2; ++d) {
      if (!(dir_mask & (1 << d))) continue;
      epi.bias = bias + d * g4;
      const int rc = ma_gemm_bf16(xb + t0[d] * B * Kpad, Kpad, wih + d * g4 * Kpad, Kpad, projbuf[d], g4, n * B, g4, Kpad, &epi, stream);
      if (rc != MA_OK) return rc;
    }
    for (int64_t s = s0; s < s0 + n; ++s) {
      LstmStepT<TAPE> p;
      const int64_t t[2] = {s, T - 1 - s};
      if constexpr (TAPE) {
        for (int d = 0; d < 2; ++d) {
          p.tape_act[d] = reinterpret_cast<float*>(reinterpret_cast<char*>(tape) + tl.act) + (d * T + t[d]) * 5 * bh;
          p.tape_h[d] = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(tape) + tl.h) + (d * T + t[d]) * bh;
        }
      }
      p.whh = reinterpret_cast<const uint16_t*>(whh_packed);
      p.h_in = hbuf + (s & 1) * 2 * bh;
      p.h_out = hbuf + ((s + 1) & 1) * 2 * bh;
      p.c = c;
      p.tie = reinterpret_cast<float*>(base + ws.tie);
      p.dir0 = dir_mask == 2 ? 1 : 0;
      p.B = (int32_t)B;
      p.H = H;
      for (int d = 0; d < 2; ++d) {
        p.proj[d] = projbuf[d] + (t[d] - t0[d]) * B * g4;
        p.out_f32[d] = out_f32 + t[d] * bh;
        p.out_bf16[d] = obf ? obf + t[d] * bh : nullptr;
        const int64_t other = T - 1 - s;  // the step at which the other direction serves this frame
        p.mode[d] = !both ? kLstmAlone : s < other ? kLstmFirst : s > other ? kLstmSecond : d == 0 ? kLstmFirst : kLstmTie;
      }
      if ((H / 32) % 16 == 0) MA_LAUNCH((lstm_step_ksplit_kernel<4, TAPE>), grid, dim3(kLstmThreads), 0, st, p);
      else if ((H / 32) % 8 == 0) MA_LAUNCH((lstm_step_ksplit_kernel<2, TAPE>), grid, dim3(kLstmThreads), 0, st, p);
      else if ((H / 32) % 4 == 0) MA_LAUNCH((lstm_step_ksplit_kernel<1, TAPE>), grid, dim3(kLstmThreads), 0, st, p);
      else MA_LAUNCH((lstm_step_kernel<2, TAPE>), grid, dim3(kLstmThreads), 0, st, p);
      if (both && s == T - 1 - s)
        MA_LAUNCH(lstm_tie_kernel, dim3((unsigned)((bh + 255) / 256)), dim3(256), 0, st, p.out_f32[0], p.out_bf16[0], p.tie, bh);
    }
  }
  if (c_final && hipMemcpyAsync(c_final, c, (size_t)(2 * bh * 4), hipMemcpyDeviceToDevice, st) != hipSuccess) return MA_ERR_LAUNCH;
  return MA_OK;
}

}  // namespace ma

extern "C" {

int ma_lstm_bidir_bf16(const void* x, int64_t T, int64_t B, int32_t Kpad, int32_t H, const void* wih_bf16, const void* whh_packed,
                       const float* bias, int32_t dir_mask, int64_t time_chunk, float* out_f32, void* out_bf16, float* c_final,
                       void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  return lstm_bidir_run<false>(x, T, B, Kpad, H, wih_bf16, whh_packed, bias, dir_mask, time_chunk, out_f32, out_bf16, c_final, nullptr, 0,
                               workspace, workspace_bytes, stream);
}

int64_t ma_lstm_train_tape_bytes(int64_t T, int64_t B, int32_t H) {
  if (T < 1 || B < 1 || H < 1) return MA_ERR_INVALID_ARG;
  if (!lstm_shape_ok(T, B, 64, H)) return MA_ERR_UNSUPPORTED;
  return lstm_tape_layout(T, B, H).total;
}

int64_t ma_lstm_train_tape_h_offset(int64_t T, int64_t B, int32_t H) {
  if (T < 1 || B < 1 || H < 1) return MA_ERR_INVALID_ARG;
  if (!lstm_shape_ok(T, B, 64, H)) return MA_ERR_UNSUPPORTED;
  return lstm_tape_layout(T, B, H).h;
}

int ma_lstm_bidir_train_bf16(const void* x, int64_t T, int64_t B, int32_t Kpad, int32_t H, const void* wih_bf16, const void* whh_packed,
                             const float* bias, int32_t dir_mask, int64_t time_chunk, float* out_f32, void* out_bf16, float* c_final,
                             void* tape, int64_t tape_bytes, void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  return lstm_bidir_run<true>(x, T, B, Kpad, H, wih_bf16, whh_packed, bias, dir_mask, time_chunk, out_f32, out_bf16, c_final, tape,
                              tape_bytes, workspace, workspace_bytes, stream);
}

}  // extern "C"
