// The two ends of TasNet (mindaudio/models/tasnet.py Encoder, Separator.layer_norm and softmax, Decoder), float32.  Contract:
// include/mindaudio_amd.h.  Between them run the LSTM stack (lstm_stack.hip or lstm.hip) and the fc GEMM (ma_gemm_bf16).
//
// ma_tasnet_gated_encode_f32: one workgroup per segment row (b, k) of mixture (B, K, L).  The row is staged in LDS, its L2 norm comes
//   from one wave reduction, each thread then runs the two length-L dot products of its basis indices n (the weights transposed to
//   (L, N), so that a wave reads 256 contiguous bytes per tap), and the LayerNorm over N is two workgroup reductions (mean, then the
//   centred second moment).  The normalised row is stored as bf16 into the LSTM stack's time-major input, row k * B + b.
// ma_tasnet_mask_decode_f32: one workgroup per (k, b).  The softmax over speakers times mixture_w goes to LDS as source_w (nspk, N);
//   each wave then runs the length-N dot products of its share of the nspk * L outputs against basis_signals (L, N), adds the bias,
//   multiplies by norm_coef (bias included, as the reference does) and stores transposed into (B, nspk, K, L).
// Every sum has a fixed order: no atomics, the same bits from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kTasThreads = 256;
constexpr int kTasMaxL = 64;
constexpr int kTasMaxN = 1024;
constexpr int kTasMaxSpk = 4;
constexpr float kTasEps = 1e-8f;  // tasnet.py:5

// sum over the workgroup's 256 threads, the same value in every thread; `red` holds 4 floats and is free again on return
__device__ __forceinline__ float tas_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kTasThreads) void tasnet_gated_encode_kernel(const float* __restrict__ mixture, int64_t B, int64_t K, int L, int N,
                                                                         const float* __restrict__ Ut, const float* __restrict__ bU,
                                                                         const float* __restrict__ Vt, const float* __restrict__ bV,
                                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                         float ln_eps, float* __restrict__ mixture_w,
                                                                         float* __restrict__ norm_coef, uint16_t* __restrict__ xin, int Kpad) {
  __shared__ float xs[kTasMaxL];
  __shared__ float red[4];
  const int64_t row = blockIdx.x;  // b * K + k
  const int64_t b = row / K, k = row - b * K;
  const int tid = threadIdx.x;
  const float v = tid < L ? mixture[row * L + tid] : 0.0f;
  const float norm = sqrtf(tas_block_sum(v * v, red));  // (L <= 64: wave 0 holds every term, the other waves add zeros)
  if (tid < L) xs[tid] = v / (norm + kTasEps);
  if (tid == 0) norm_coef[row] = norm;
  __syncthreads();

  float w[kTasMaxN / kTasThreads];
  float sum = 0.0f;
#pragma unroll
  for (int i = 0; i < kTasMaxN / kTasThreads; ++i) {
    const int n = tid + i * kTasThreads;
    w[i] = 0.0f;
    if (n < N) {
      float u = bU[n], g = bV[n];
      for (int j = 0; j < L; ++j) {
        u = fmaf(xs[j], Ut[(int64_t)j * N + n], u);
        g = fmaf(xs[j], Vt[(int64_t)j * N + n], g);
      }
      w[i] = fmaxf(u, 0.0f) * (1.0f / (1.0f + expf(-g)));
      mixture_w[row * N + n] = w[i];
      sum += w[i];
    }
  }
  const float mean = tas_block_sum(sum, red) / (float)N;
  float m2 = 0.0f;
#pragma unroll
  for (int i = 0; i < kTasMaxN / kTasThreads; ++i) {
    const int n = tid + i * kTasThreads;
    if (n < N) m2 += (w[i] - mean) * (w[i] - mean);
  }
  const float rstd = 1.0f / sqrtf(tas_block_sum(m2, red) / (float)N + ln_eps);
  uint16_t* dst = xin + (k * B + b) * Kpad;
#pragma unroll
  for (int i = 0; i < kTasMaxN / kTasThreads; ++i) {
    const int n = tid + i * kTasThreads;
    if (n < N) dst[n] = f2bf((w[i] - mean) * rstd * gamma[n] + beta[n]);
  }
}

__global__ __launch_bounds__(kTasThreads) void tasnet_mask_decode_kernel(const float* __restrict__ score, int64_t ld_score,
                                                                        const float* __restrict__ mixture_w,
                                                                        const float* __restrict__ norm_coef, int64_t B, int64_t K, int nspk,
                                                                        int N, const float* __restrict__ basis, const float* __restrict__ bias,
                                                                        int L, float* __restrict__ out) {
  __shared__ float sw[kTasMaxSpk * kTasMaxN];  // source_w (nspk, N)
  const int64_t r = blockIdx.x;                // k * B + b: the fc output's row
  const int64_t k = r / B, b = r - k * B;
  const int64_t row = b * K + k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* sc = score + r * ld_score;
  for (int n = tid; n < N; n += kTasThreads) {
    float e[kTasMaxSpk];  // (constant trip counts: the array stays in registers)
    float mx = sc[n];
#pragma unroll
    for (int s = 1; s < kTasMaxSpk; ++s)
      if (s < nspk) mx = fmaxf(mx, sc[(int64_t)s * N + n]);
    float den = 0.0f;
#pragma unroll
    for (int s = 0; s < kTasMaxSpk; ++s) {
      e[s] = s < nspk ? expf(sc[(int64_t)s * N + n] - mx) : 0.0f;
      den += e[s];
    }
    const float mw = mixture_w[row * N + n];
#pragma unroll
    for (int s = 0; s < kTasMaxSpk; ++s)
      if (s < nspk) sw[s * N + n] = mw * (e[s] / den);
  }
  __syncthreads();
  const float coef = norm_coef[row];
  for (int o = wave; o < nspk * L; o += kTasThreads / 64) {
    const int s = o / L, l = o - s * L;
    const float* bs = basis + (int64_t)l * N;
    float acc = 0.0f;
    for (int n = lane; n < N; n += 64) acc = fmaf(sw[s * N + n], bs[n], acc);
    acc = wave_sum(acc);
    if (lane == 0) out[((b * nspk + s) * K + k) * L + l] = (acc + bias[l]) * coef;
  }
}

}  // namespace ma

using namespace ma;

extern "C" {

int ma_tasnet_gated_encode_f32(const float* mixture, int64_t B, int64_t K, int32_t L, int32_t N, const float* Ut, const float* bU,
                               const float* Vt, const float* bV, const float* gamma, const float* beta, float ln_eps, float* mixture_w,
                               float* norm_coef, void* xin, int32_t Kpad, ma_stream_t stream) {
  if (!mixture || !Ut || !bU || !Vt || !bV || !gamma || !beta || !mixture_w || !norm_coef || !xin || B < 1 || K < 1 || L < 1 || N < 1 ||
      Kpad < N || !(ln_eps >= 0.0f))
    return MA_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(mixture) | reinterpret_cast<uintptr_t>(mixture_w) | reinterpret_cast<uintptr_t>(xin)) & 15)
    return MA_ERR_INVALID_ARG;
  if (L > kTasMaxL || N > kTasMaxN || B * K > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(tasnet_gated_encode_kernel, dim3((unsigned)(B * K)), dim3(kTasThreads), 0, (hipStream_t)stream, mixture, B, K, L, N, Ut, bU, Vt,
            bV, gamma, beta, ln_eps, mixture_w, norm_coef, reinterpret_cast<uint16_t*>(xin), Kpad);
  return MA_OK;
}

int ma_tasnet_mask_decode_f32(const float* score, int64_t ld_score, const float* mixture_w, const float* norm_coef, int64_t B, int64_t K,
                              int32_t nspk, int32_t N, const float* basis, const float* bias, int32_t L, float* out, ma_stream_t stream) {
  if (!score || !mixture_w || !norm_coef || !basis || !bias || !out || B < 1 || K < 1 || nspk < 1 || N < 1 || L < 1 ||
      ld_score < (int64_t)nspk * N)
    return MA_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(score) | reinterpret_cast<uintptr_t>(mixture_w) | reinterpret_cast<uintptr_t>(out)) & 15)
    return MA_ERR_INVALID_ARG;
  if (nspk > kTasMaxSpk || L > kTasMaxL || N > kTasMaxN || B * K > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(tasnet_mask_decode_kernel, dim3((unsigned)(B * K)), dim3(kTasThreads), 0, (hipStream_t)stream, score, ld_score, mixture_w,
            norm_coef, B, K, nspk, N, basis, bias, L, out);
  return MA_OK;
}

}  // extern "C"
