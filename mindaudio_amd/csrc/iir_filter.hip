// IIR filters of mindaudio/data/filters.py (cal_filter_by_coffs: the biquad behind low_pass_filter and peaking_equalizer; filtfilt:
// scipy.signal.butter + scipy.signal.filtfilt).  Contract: include/mindaudio_amd.h.
//
// The reference walks every sample of every channel in a Python loop.  The recursion is the transposed direct form II SciPy uses,
//   y = b0 x + z0,   z_i = b_(i+1) x + z_(i+1) - a_(i+1) y   (z_n = 0),
// which is linear in (state, input): a row is cut into chunks of L samples whose carries compose.
//   1. iir_chunk_kernel<.., false>: every chunk but a row's last one runs from a zero state; its final state s_c is kept.
//   2. iir_carry_kernel: one wave per row walks the chunks in order, z_(c+1) = P z_c + s_c with P = A^L from the host, and leaves
//      the true state z_c where s_c was.
//   3. iir_chunk_kernel<.., true>: every chunk runs again from its true state and writes its samples.  Inside a chunk this is the
//      sequential recursion itself, so chunking changes the rounding through the carried state only.
// One chunk per row (the plan of an unstable or ill-conditioned filter, data/filters.py iir_plan) is step 3 alone: the reference's
// order, one thread per row.
//
// A thread owns a chunk, neighbouring lanes own neighbouring chunks (of the same row, then of the next one), so a lane's samples are
// L apart from its neighbour's.  They are staged through LDS kIirTile samples at a time: half a wave reads or writes kIirTile
// consecutive samples of one chunk, and the tile's row stride kIirTile + 1 is odd, so that both the staging accesses (consecutive
// words) and the recursion's (one row per lane) spread over all banks.  One wave per workgroup: the barriers cost nothing and 17 KiB
// of LDS (float64 samples) leave room for nine workgroups per CU.
//
// Coefficients, state and arithmetic are float64; samples float32 or float64.  The order is padded with zero coefficients to 2, 4, 8
// or 16 (a zero tap adds b x + 0 - 0 y = the exact value the shorter recursion has).  No atomics, every sum in index order: the same
// bits from run to run, and for a row alone or inside a batch (a chunk never meets another one).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kIirLanes = 64;  // chunks per workgroup
constexpr int kIirTile = 32;   // samples of every chunk staged at a time
static_assert(kIirLanes == 2 * kIirTile, "a staging pass moves one tile row per half wave");

// by value in the kernel arguments: uniform, read with scalar loads at constant offsets once the loops over taps are unrolled
struct IirCoef {
  double b[MA_IIR_MAX_ORDER + 1];
  double a[MA_IIR_MAX_ORDER + 1];
  double zi[MA_IIR_MAX_ORDER];
};
template <int N>
struct IirPower {
  double p[N * N];  // row-major A^L
};

// Where a chunk's samples live: processing position p of the chunk is element base + dir * p (dir = -1 walks the row backwards).
// y may be x: a workgroup has read the samples of a tile before it writes them.
template <typename S, int N, bool kEmit>
__global__ __launch_bounds__(kIirLanes) void iir_chunk_kernel(const S* x, S* y, int64_t chunks, int T, int L,
                                                              int C, IirCoef k, int zi_mode, int reverse, int upper_clamp,
                                                              double* __restrict__ ws) {
  __shared__ S tile[kIirLanes][kIirTile + 1];
  __shared__ int64_t chunk_base[kIirLanes];
  __shared__ int chunk_len[kIirLanes];
  const int lane = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kIirLanes + lane;  // chunk c of row g / C
  const int dir = reverse ? -1 : 1;
  int len = 0;
  int64_t base = 0;
  bool keep = false;  // step 1: this chunk's final state is carried forward
  if (g < chunks) {
    const int64_t row = g / C;
    const int c = (int)(g - row * C);
    const int start = c * L;  // (C - 1) * L < T
    len = min(L, T - start);
    base = row * (int64_t)T + (reverse ? T - 1 - start : start);
    keep = c < C - 1;
    if (!kEmit && !keep) len = 0;  // a row's last chunk carries nothing forward
  }
  chunk_base[lane] = base;
  chunk_len[lane] = len;

  double z[N];
#pragma unroll
  for (int i = 0; i < N; ++i) z[i] = 0.0;
  if (kEmit && len > 0) {
    if (C > 1) {
#pragma unroll
      for (int i = 0; i < N; ++i) z[i] = ws[g * N + i];
    } else if (zi_mode != MA_IIR_ZI_NONE) {
      const double x0 = zi_mode == MA_IIR_ZI_TIMES_X0 ? (double)x[base] : 1.0;
#pragma unroll
      for (int i = 0; i < N; ++i) z[i] = k.zi[i] * x0;
    }
  }
  __syncthreads();

  // lane -> (chunk, sample) of the staging accesses: pass `it` moves samples [0, kIirTile) of chunks 2 it and 2 it + 1
  const int half = lane / kIirTile, s_st = lane % kIirTile;
  const int longest = min(L, T);
  for (int s0 = 0; s0 < longest; s0 += kIirTile) {
    {  // every load is issued before the first one is waited for
      S staged[kIirLanes / 2];
#pragma unroll
      for (int it = 0; it < kIirLanes / 2; ++it) {
        const int ch = 2 * it + half;
        staged[it] = s0 + s_st < chunk_len[ch] ? x[chunk_base[ch] + (int64_t)dir * (s0 + s_st)] : (S)0;
      }
#pragma unroll
      for (int it = 0; it < kIirLanes / 2; ++it) tile[2 * it + half][s_st] = staged[it];
    }
    __syncthreads();
    if (s0 < len) {
      S mine[kIirTile];  // the lane's samples of this tile, read before the recursion's chain starts
#pragma unroll
      for (int s = 0; s < kIirTile; ++s) mine[s] = tile[lane][s];
      if (s0 + kIirTile <= len) {
#pragma unroll
        for (int s = 0; s < kIirTile; ++s) {
          const double xv = (double)mine[s];
          const double yv = fma(k.b[0], xv, z[0]);
#pragma unroll
          for (int i = 0; i < N - 1; ++i) z[i] = fma(-k.a[i + 1], yv, fma(k.b[i + 1], xv, z[i + 1]));
          z[N - 1] = fma(-k.a[N], yv, k.b[N] * xv);
          if (kEmit) tile[lane][s] = (S)(upper_clamp && yv > 1.0 ? 1.0 : yv);  // the recursion goes on from the unclamped value
        }
      } else {  // the ragged end of a row: the same operations, sample by sample
        for (int s = 0; s < len - s0; ++s) {
          const double xv = (double)tile[lane][s];
          const double yv = fma(k.b[0], xv, z[0]);
#pragma unroll
          for (int i = 0; i < N - 1; ++i) z[i] = fma(-k.a[i + 1], yv, fma(k.b[i + 1], xv, z[i + 1]));
          z[N - 1] = fma(-k.a[N], yv, k.b[N] * xv);
          if (kEmit) tile[lane][s] = (S)(upper_clamp && yv > 1.0 ? 1.0 : yv);
        }
      }
    }
    __syncthreads();
    if (kEmit) {
#pragma unroll
      for (int it = 0; it < kIirLanes / 2; ++it) {
        const int ch = 2 * it + half;
        if (s0 + s_st < chunk_len[ch]) y[chunk_base[ch] + (int64_t)dir * (s0 + s_st)] = tile[ch][s_st];
      }
      __syncthreads();
    }
  }
  if (!kEmit && keep) {
#pragma unroll
    for (int i = 0; i < N; ++i) ws[g * N + i] = z[i];
  }
}

// One wave per row.  Slot c of the row's workspace holds s_c on entry (slot C - 1: nothing) and z_c on exit.  Lane i < N owns
// component i of the state and row i of P; the chunks' slots pass through LDS 64 at a time, so global memory is touched in runs.
template <typename S, int N>
__global__ __launch_bounds__(kIirLanes) void iir_carry_kernel(const S* __restrict__ x, int T, int C, IirCoef k, IirPower<N> pw,
                                                              int zi_mode, int reverse, double* __restrict__ ws) {
  __shared__ double slots[(kIirLanes + 1) * N];
  const int lane = threadIdx.x;
  const int i = lane < N ? lane : 0;
  const int64_t row = blockIdx.x;
  double* w = ws + row * (int64_t)C * N;
  double prow[N];
#pragma unroll
  for (int j = 0; j < N; ++j) prow[j] = pw.p[i * N + j];
  double z = 0.0;
  if (zi_mode != MA_IIR_ZI_NONE) {
    const double x0 = zi_mode == MA_IIR_ZI_TIMES_X0 ? (double)x[row * (int64_t)T + (reverse ? T - 1 : 0)] : 1.0;
    z = k.zi[i] * x0;
  }
  for (int c0 = 0; c0 < C; c0 += kIirLanes) {
    const int nb = min(kIirLanes, C - c0);
    for (int e = lane; e < nb * N; e += kIirLanes) slots[e] = w[(int64_t)c0 * N + e];
    __syncthreads();
    double sv = slots[i];
    for (int u = 0; u < nb; ++u) {
      const double sv_next = slots[(u + 1) * N + i];  // (one spare row: read, never used, after the last chunk)
      if (lane < N) slots[u * N + i] = z;
      if (c0 + u < C - 1) {
        // component j of the state, from lane j: two scalar lane reads, no trip through LDS
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const double zj = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(z), j),
                                             __builtin_amdgcn_readlane(__double2loint(z), j));
          acc = j == 0 ? prow[0] * zj : fma(prow[j], zj, acc);
        }
        z = acc + sv;
      }
      sv = sv_next;
    }
    __syncthreads();
    for (int e = lane; e < nb * N; e += kIirLanes) w[(int64_t)c0 * N + e] = slots[e];
    __syncthreads();
  }
}

static int iir_padded_order(int n) { return n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16; }

template <typename S, int N>
static int iir_launch(const S* x, S* y, int64_t rows, int T, int L, int C, const ma_iir_filter_t& f, double* ws, hipStream_t stream) {
  IirCoef k = {};
  for (int i = 0; i <= f.order; ++i) {
    k.b[i] = f.b[i];
    k.a[i] = f.a[i];
  }
  const int zi_mode = f.zi ? f.zi_mode : MA_IIR_ZI_NONE;
  if (zi_mode != MA_IIR_ZI_NONE)
    for (int i = 0; i < f.order; ++i) k.zi[i] = f.zi[i];
  const int64_t chunks = rows * C;
  const dim3 grid((unsigned)((chunks + kIirLanes - 1) / kIirLanes));
  const int steps = f.steps ? f.steps : MA_IIR_STEP_CHUNK_STATES | MA_IIR_STEP_CARRY | MA_IIR_STEP_EMIT;
  if (C > 1) {
    IirPower<N> pw = {};
    for (int i = 0; i < f.order; ++i)
      for (int j = 0; j < f.order; ++j) pw.p[i * N + j] = f.power[i * f.order + j];
    if (steps & MA_IIR_STEP_CHUNK_STATES)
      MA_LAUNCH((iir_chunk_kernel<S, N, false>), grid, dim3(kIirLanes), 0, stream, x, y, chunks, T, L, C, k, zi_mode, f.reverse,
                f.upper_clamp, ws);
    if (steps & MA_IIR_STEP_CARRY)
      MA_LAUNCH((iir_carry_kernel<S, N>), dim3((unsigned)rows), dim3(kIirLanes), 0, stream, x, T, C, k, pw, zi_mode, f.reverse, ws);
  }
  if (steps & MA_IIR_STEP_EMIT)
    MA_LAUNCH((iir_chunk_kernel<S, N, true>), grid, dim3(kIirLanes), 0, stream, x, y, chunks, T, L, C, k, zi_mode, f.reverse,
              f.upper_clamp, ws);
  return MA_OK;
}

template <typename S>
static int iir_dispatch(const void* x, void* y, int64_t rows, int T, int L, int C, const ma_iir_filter_t& f, void* ws,
                        hipStream_t stream) {
  const S* xs = static_cast<const S*>(x);
  S* ys = static_cast<S*>(y);
  double* w = static_cast<double*>(ws);
  switch (iir_padded_order(f.order)) {
    case 2: return iir_launch<S, 2>(xs, ys, rows, T, L, C, f, w, stream);
    case 4: return iir_launch<S, 4>(xs, ys, rows, T, L, C, f, w, stream);
    case 8: return iir_launch<S, 8>(xs, ys, rows, T, L, C, f, w, stream);
    default: return iir_launch<S, 16>(xs, ys, rows, T, L, C, f, w, stream);
  }
}

}  // namespace ma

using namespace ma;

extern "C" int64_t ma_iir_filter_workspace_bytes(int64_t rows, int64_t T, int32_t order, int64_t chunk) {
  if (rows < 1 || T < 1 || order < 1 || order > MA_IIR_MAX_ORDER || chunk < 1) return 0;
  const int64_t C = (T + chunk - 1) / chunk;
  return C > 1 ? rows * C * iir_padded_order(order) * (int64_t)sizeof(double) : 0;
}

extern "C" int ma_iir_filter(const void* x, int32_t sample_bytes, int64_t rows, int64_t T, const ma_iir_filter_t* filter, void* y,
                             void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  if (!x || !y || !filter || rows < 1 || T < 1 || (sample_bytes != 4 && sample_bytes != 8)) return MA_ERR_INVALID_ARG;
  const ma_iir_filter_t& f = *filter;
  if (f.order < 1 || f.chunk < 1 || !f.b || !f.a) return MA_ERR_INVALID_ARG;
  if (f.order > MA_IIR_MAX_ORDER) return MA_ERR_UNSUPPORTED;
  if (f.a[0] != 1.0) return MA_ERR_INVALID_ARG;
  if (f.zi_mode != MA_IIR_ZI_NONE && f.zi_mode != MA_IIR_ZI_AS_IS && f.zi_mode != MA_IIR_ZI_TIMES_X0) return MA_ERR_INVALID_ARG;
  if (f.steps & ~(MA_IIR_STEP_CHUNK_STATES | MA_IIR_STEP_CARRY | MA_IIR_STEP_EMIT)) return MA_ERR_INVALID_ARG;
  if (T > 0x7fffff00) return MA_ERR_UNSUPPORTED;
  const int64_t L = f.chunk < T ? f.chunk : T, C = (T + L - 1) / L;
  if (C > 1 && !f.power) return MA_ERR_INVALID_ARG;
  if (rows > 0x7fffffff || rows * C > (int64_t)0x7fffffff * kIirLanes) return MA_ERR_UNSUPPORTED;
  if (C > 1) {
    const int64_t need = ma_iir_filter_workspace_bytes(rows, T, f.order, L);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)) return MA_ERR_WORKSPACE;
  }
  if (sample_bytes == 4) return iir_dispatch<float>(x, y, rows, (int)T, (int)L, (int)C, f, workspace, (hipStream_t)stream);
  return iir_dispatch<double>(x, y, rows, (int)T, (int)L, (int)C, f, workspace, (hipStream_t)stream);
}
