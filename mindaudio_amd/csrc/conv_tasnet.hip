// Conv-TasNet separation (mindaudio/models/conv_tasnet.py, mindaudio/loss/separation_loss.py): everything between the 1 x 1
// convolutions, which are ma_gemm_bf16 calls.  Contract: include/mindaudio_amd.h.
//
// Layout: an activation is (M * K, channels) float32, channels contiguous, utterance m owns the rows [m * K, (m + 1) * K) and there
// are no halo rows: the depthwise kernel checks every tap against its own utterance's [0, K).  A wave reads 64 (x 4) neighbouring
// channels of one row, so the three rows of a tap set are three coalesced reads.
//
// Global layer norm needs the mean and variance of a whole utterance (all channels, all frames).  Every kernel that PRODUCES a
// tensor which is normalised next leaves, per workgroup, the centred float64 moments of its tile (count, sum, sum of (v - tile mean)^2;
// the tile is still in registers for the second pass); every kernel that CONSUMES the tensor joins its utterance's partials itself, in
// index order (Chan's update: M2 = sum M2_p + n_p (mean_p - mean)^2), which saves a finalize launch.  No atomics anywhere: the same
// bits from run to run.  The variance never goes through E[v^2] - mean^2, so it cannot cancel.
//
// A tile is 8192 / C rows of one utterance (grid = (tiles per utterance, M)); a thread owns at most 32 values.
//
// bf16 appears in ma_gln_apply_bf16 only (the operand of the next GEMM); everything else here is float32 with float64 statistics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"
#include "tasnet_common.h"

namespace ma {

// ---- encoder: mixture_w[m, k, n] = relu(sum_j x[m, k * hop + j] * Wt[j, n]) ------------------------------------------------------------
__global__ __launch_bounds__(kTnThreads) void tasnet_encode_kernel(const float* __restrict__ x, int64_t T, int64_t ldx, int64_t K,
                                                                   const float* __restrict__ Wt, int L, int N, int rows,
                                                                   float* __restrict__ mw, double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t m = blockIdx.y, row0 = (int64_t)blockIdx.x * rows;
  const int rows_here = K - row0 < rows ? (int)(K - row0) : rows;
  const int count = rows_here * N, hop = L / 2;
  const float* xm = x + m * ldx;
  float* o = mw + (m * K + row0) * N;
  float v[kTnTileElems / kTnThreads];
  double ts = 0.0;
#pragma unroll
  for (int i = 0; i < kTnTileElems / kTnThreads; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    v[i] = 0.0f;
    if (e < count) {
      const int r = e / N, n = e - r * N;
      const float* xr = xm + (row0 + r) * hop;  // (row0 + r) * hop + L - 1 <= (K - 1) * hop + L - 1 < T
      float acc = 0.0f;
      for (int j = 0; j < L; ++j) acc = fmaf(xr[j], Wt[(int64_t)j * N + n], acc);
      acc = fmaxf(acc, 0.0f);
      v[i] = acc;
      o[e] = acc;
      ts += (double)acc;
    }
  }
  tile_moments(ts, count, sh, part + (m * gridDim.x + blockIdx.x) * 3, [&](double mean) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < kTnTileElems / kTnThreads; ++i)
      if (threadIdx.x + i * kTnThreads < count) {
        const double d = (double)v[i] - mean;
        q += d * d;
      }
    return q;
  });
}

// ---- PReLU of a GEMM output + the moments of the result ------------------------------------------------------------------------------
// (x and y carry no __restrict__: y may be x - each thread reads its elements before it writes them)
__global__ __launch_bounds__(kTnThreads) void prelu_gln_stats_kernel(const float* x, int64_t K, int C, int rows,
                                                                     const float* __restrict__ a_ptr, float* y,
                                                                     double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t m = blockIdx.y, row0 = (int64_t)blockIdx.x * rows;
  const int rows_here = K - row0 < rows ? (int)(K - row0) : rows;
  const int n4 = rows_here * (C / 4);
  const int64_t base = (m * K + row0) * C;
  const float a = a_ptr[0];
  float4 v[kTnIter4];
  double ts = 0.0;
#pragma unroll
  for (int i = 0; i < kTnIter4; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (e < n4) {
      float4 t = *reinterpret_cast<const float4*>(x + base + (int64_t)e * 4);
      t.x = prelu(t.x, a);
      t.y = prelu(t.y, a);
      t.z = prelu(t.z, a);
      t.w = prelu(t.w, a);
      *reinterpret_cast<float4*>(y + base + (int64_t)e * 4) = t;
      v[i] = t;
      ts += ((double)t.x + (double)t.y) + ((double)t.z + (double)t.w);
    }
  }
  tile_moments(ts, (int64_t)n4 * 4, sh, part + (m * gridDim.x + blockIdx.x) * 3, [&](double mean) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < kTnIter4; ++i)
      if (threadIdx.x + i * kTnThreads < n4) {
        const double d0 = (double)v[i].x - mean, d1 = (double)v[i].y - mean, d2 = (double)v[i].z - mean, d3 = (double)v[i].w - mean;
        q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
    return q;
  });
}

// ---- gLN -> depthwise dilated conv (3 taps, zero padding of the NORMALISED values) -> PReLU + the moments of the result ----------------
__global__ __launch_bounds__(kTnThreads) void gln_dwconv_prelu_kernel(const float* __restrict__ y, int64_t K, int C, int rows,
                                                                      const double* __restrict__ part_in, int nparts_in,
                                                                      const float* __restrict__ Wt, int dil,
                                                                      const float* __restrict__ a_ptr, float* __restrict__ z,
                                                                      double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t m = blockIdx.y, row0 = (int64_t)blockIdx.x * rows;
  const int rows_here = K - row0 < rows ? (int)(K - row0) : rows;
  const int C4 = C / 4, n4 = rows_here * C4;
  const int64_t base = (m * K + row0) * C;
  float mean, rstd;
  gln_mean_rstd(part_in + m * nparts_in * 3, nparts_in, sh, mean, rstd);
  const float a = a_ptr[0];
  const int64_t step = (int64_t)dil * C;
  float4 v[kTnIter4];
  double ts = 0.0;
#pragma unroll
  for (int i = 0; i < kTnIter4; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (e < n4) {
      const int r = e / C4, c = (e - r * C4) * 4;
      const int64_t k = row0 + r;  // frame inside the utterance
      const float* p = y + base + (int64_t)e * 4;
      const float4 w0 = *reinterpret_cast<const float4*>(Wt + c);
      const float4 w1 = *reinterpret_cast<const float4*>(Wt + C + c);
      const float4 w2 = *reinterpret_cast<const float4*>(Wt + 2 * C + c);
      float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (k - dil >= 0) {
        const float4 q = *reinterpret_cast<const float4*>(p - step);
        t.x = w0.x * ((q.x - mean) * rstd);
        t.y = w0.y * ((q.y - mean) * rstd);
        t.z = w0.z * ((q.z - mean) * rstd);
        t.w = w0.w * ((q.w - mean) * rstd);
      }
      {
        const float4 q = *reinterpret_cast<const float4*>(p);
        t.x = fmaf(w1.x, (q.x - mean) * rstd, t.x);
        t.y = fmaf(w1.y, (q.y - mean) * rstd, t.y);
        t.z = fmaf(w1.z, (q.z - mean) * rstd, t.z);
        t.w = fmaf(w1.w, (q.w - mean) * rstd, t.w);
      }
      if (k + dil < K) {
        const float4 q = *reinterpret_cast<const float4*>(p + step);
        t.x = fmaf(w2.x, (q.x - mean) * rstd, t.x);
        t.y = fmaf(w2.y, (q.y - mean) * rstd, t.y);
        t.z = fmaf(w2.z, (q.z - mean) * rstd, t.z);
        t.w = fmaf(w2.w, (q.w - mean) * rstd, t.w);
      }
      t.x = prelu(t.x, a);
      t.y = prelu(t.y, a);
      t.z = prelu(t.z, a);
      t.w = prelu(t.w, a);
      *reinterpret_cast<float4*>(z + base + (int64_t)e * 4) = t;
      v[i] = t;
      ts += ((double)t.x + (double)t.y) + ((double)t.z + (double)t.w);
    }
  }
  tile_moments(ts, (int64_t)n4 * 4, sh, part + (m * gridDim.x + blockIdx.x) * 3, [&](double mu) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < kTnIter4; ++i)
      if (threadIdx.x + i * kTnThreads < n4) {
        const double d0 = (double)v[i].x - mu, d1 = (double)v[i].y - mu, d2 = (double)v[i].z - mu, d3 = (double)v[i].w - mu;
        q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
    return q;
  });
}

// ---- gLN -> bf16, the operand of the next 1 x 1 convolution -----------------------------------------------------------------------------
__global__ __launch_bounds__(kTnThreads) void gln_apply_bf16_kernel(const float* __restrict__ y, int64_t K, int C, int rows,
                                                                    const double* __restrict__ part_in, int nparts_in,
                                                                    uint16_t* __restrict__ out) {
  __shared__ double sh[4];
  const int64_t m = blockIdx.y, row0 = (int64_t)blockIdx.x * rows;
  const int rows_here = K - row0 < rows ? (int)(K - row0) : rows;
  const int n4 = rows_here * (C / 4);
  const int64_t base = (m * K + row0) * C;
  float mean, rstd;
  gln_mean_rstd(part_in + m * nparts_in * 3, nparts_in, sh, mean, rstd);
#pragma unroll
  for (int i = 0; i < kTnIter4; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    if (e < n4) {
      const float4 q = *reinterpret_cast<const float4*>(y + base + (int64_t)e * 4);
      uint2 o;
      o.x = (uint32_t)f2bf((q.x - mean) * rstd) | ((uint32_t)f2bf((q.y - mean) * rstd) << 16);
      o.y = (uint32_t)f2bf((q.z - mean) * rstd) | ((uint32_t)f2bf((q.w - mean) * rstd) << 16);
      *reinterpret_cast<uint2*>(out + base + (int64_t)e * 4) = o;
    }
  }
}

// ---- decoder: mask, basis signals and the overlap in one launch --------------------------------------------------------------------------
// out (M, C, (K + 1) * hop) is (K + 1) segments of hop samples.  With frame_k[l] = sum_n relu(score[m, k, c * N + n]) * mw[m, k, n] *
// basis[l, n] (0 outside 0 <= k < K):
//   paired (the reference's 0 / 1 matrix product):  segment k = frame_k[j] + frame_k[j + hop]       (segment K: the zero pad)
//   true overlap-add:                               segment k = frame_k[j] + frame_{k-1}[j + hop]
// A wave owns kDecSeg neighbouring segments of one (m, c) and computes the kDecSeg + 1 frames they need (the first one again, for the
// true overlap); lane i keeps the products for n = i, i + 64, ... in its own slots of LDS, each basis row is read once per wave and
// dotted with all frames, and a butterfly sum leaves frame[l] in lane l.
constexpr int kDecSeg = 4;
constexpr int kDecFrames = kDecSeg + 1;

__global__ __launch_bounds__(kTnThreads) void tasnet_decode_kernel(const float* __restrict__ score, const float* __restrict__ mw,
                                                                   int64_t K, int C, int N, const float* __restrict__ basis, int L,
                                                                   int true_overlap, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float dec_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NI = N / 64, hop = L / 2;
  float* s = dec_lds + (int64_t)wave * kDecFrames * N;  // [frame][i][lane]: only ever read by the lane that wrote it
  const int64_t mc = blockIdx.y, m = mc / C, c = mc - m * C;
  const int64_t k0 = ((int64_t)blockIdx.x * (kTnThreads / 64) + wave) * kDecSeg;  // first segment of the wave
  if (k0 > K) return;  // (nothing below synchronises across waves)
#pragma unroll
  for (int f = 0; f < kDecFrames; ++f) {
    const int64_t k = k0 - 1 + f;
    const bool live = k >= 0 && k < K && (f > 0 || true_overlap);
    const float* sp = score + (m * K + k) * ((int64_t)C * N) + c * N;
    const float* wp = mw + (m * K + k) * N;
    for (int i = 0; i < NI; ++i) {
      float v = 0.0f;
      if (live) v = fmaxf(sp[i * 64 + lane], 0.0f) * wp[i * 64 + lane];
      s[(f * NI + i) * 64 + lane] = v;
    }
  }
  float mine[kDecFrames];
#pragma unroll
  for (int f = 0; f < kDecFrames; ++f) mine[f] = 0.0f;
  for (int l = 0; l < L; ++l) {
    float acc[kDecFrames];
#pragma unroll
    for (int f = 0; f < kDecFrames; ++f) acc[f] = 0.0f;
    for (int i = 0; i < NI; ++i) {
      const float w = basis[(int64_t)l * N + i * 64 + lane];
#pragma unroll
      for (int f = 0; f < kDecFrames; ++f) acc[f] = fmaf(s[(f * NI + i) * 64 + lane], w, acc[f]);
    }
#pragma unroll
    for (int f = 0; f < kDecFrames; ++f) {
      const float tot = wave_sum(acc[f]);
      mine[f] = lane == l ? tot : mine[f];
    }
  }
  float* o = out + mc * ((K + 1) * hop);
#pragma unroll
  for (int f = 1; f < kDecFrames; ++f) {
    const int64_t k = k0 - 1 + f;
    const float hi_same = __shfl(mine[f], (lane + hop) & 63, 64);
    const float hi_prev = __shfl(mine[f - 1], (lane + hop) & 63, 64);
    const float val = mine[f] + (true_overlap ? hi_prev : hi_same);
    if (k <= K && lane < hop) o[k * hop + lane] = val;
  }
}

// ---- pairwise SI-SNR (separation_loss.py:188-216) in float64 ---------------------------------------------------------------------------
// one workgroup per (b, i_est, j_target): the means over the valid samples, then the projection and the noise term by term
__global__ __launch_bounds__(kTnThreads) void si_snr_pairwise_kernel(const float* __restrict__ src, const float* __restrict__ est,
                                                                     const int64_t* __restrict__ lengths, int C, int64_t T,
                                                                     double* __restrict__ out) {
  __shared__ double sh[4];
  const int64_t id = blockIdx.x, b = id / (C * C);
  const int i = (int)((id / C) % C), j = (int)(id % C);
  const int64_t len = lengths[b] < 0 ? 0 : lengths[b] > T ? T : lengths[b];
  const float* e = est + (b * C + i) * T;
  const float* t = src + (b * C + j) * T;
  const double eps = 1e-8;
  double se = 0.0, st = 0.0;
  for (int64_t n = threadIdx.x; n < len; n += kTnThreads) {
    se += (double)e[n];
    st += (double)t[n];
  }
  const double num = (double)(len > 0 ? len : 1);  // the clamped length; an empty utterance gives 10 log10(eps) everywhere
  const double me = tile_sum(se, sh) / num, mt = tile_sum(st, sh) / num;
  double dot = 0.0, en = 0.0;
  for (int64_t n = threadIdx.x; n < len; n += kTnThreads) {
    const double a = (double)e[n] - me, r = (double)t[n] - mt;
    dot += a * r;
    en += r * r;
  }
  dot = tile_sum(dot, sh);
  en = tile_sum(en, sh) + eps;
  double pp = 0.0, nn = 0.0;
  for (int64_t n = threadIdx.x; n < len; n += kTnThreads) {
    const double a = (double)e[n] - me, r = (double)t[n] - mt;
    const double proj = dot * r / en, noise = a - proj;
    pp += proj * proj;
    nn += noise * noise;
  }
  pp = tile_sum(pp, sh);
  nn = tile_sum(nn, sh);
  if (threadIdx.x == 0) out[id] = 10.0 * log(pp / (nn + eps) + eps) / log(10.0);
}

}  // namespace ma

using namespace ma;

extern "C" int32_t ma_tasnet_stat_parts(int64_t K, int32_t C) {
  int64_t tiles = 0;
  if (check_tiles(1, K, C, &tiles) != MA_OK) return 0;
  return (int32_t)tiles;
}

extern "C" int ma_tasnet_encode_f32(const float* x, int64_t M, int64_t T, int64_t ldx, const float* Wt, int32_t L, int32_t N,
                                    float* mixture_w, double* part, ma_stream_t stream) {
  if (!x || !Wt || !mixture_w || !part || L < 2 || T < L || ldx < T) return MA_ERR_INVALID_ARG;
  if (L & 1) return MA_ERR_UNSUPPORTED;
  const int64_t K = (T - L) / (L / 2) + 1;
  int64_t tiles = 0;
  const int rc = check_tiles(M, K, N, &tiles);
  if (rc != MA_OK) return rc;
  MA_LAUNCH(tasnet_encode_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, x, T, ldx, K, Wt, L, N,
            tile_rows(N), mixture_w, part);
  return MA_OK;
}

extern "C" int ma_prelu_gln_stats(const float* x, int64_t M, int64_t K, int32_t C, const float* weight, float* y, double* part,
                                  ma_stream_t stream) {
  if (!x || !weight || !y || !part) return MA_ERR_INVALID_ARG;
  int64_t tiles = 0;
  const int rc = check_tiles(M, K, C, &tiles);
  if (rc != MA_OK) return rc;
  if (!aligned16(x) || !aligned16(y)) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(prelu_gln_stats_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, x, K, C, tile_rows(C),
            weight, y, part);
  return MA_OK;
}

extern "C" int ma_gln_dwconv_prelu(const float* y, int64_t M, int64_t K, int32_t C, const double* part_in, const float* Wt, int32_t P,
                                   int32_t dilation, const float* weight, float* z, double* part_out, ma_stream_t stream) {
  if (!y || !part_in || !Wt || !weight || !z || !part_out || P < 1 || dilation < 1 || z == y) return MA_ERR_INVALID_ARG;
  if (P != 3) return MA_ERR_UNSUPPORTED;
  int64_t tiles = 0;
  const int rc = check_tiles(M, K, C, &tiles);
  if (rc != MA_OK) return rc;
  if (!aligned16(y) || !aligned16(z) || !aligned16(Wt)) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(gln_dwconv_prelu_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, y, K, C, tile_rows(C),
            part_in, (int)tiles, Wt, dilation, weight, z, part_out);
  return MA_OK;
}

extern "C" int ma_gln_apply_bf16(const float* y, int64_t M, int64_t K, int32_t C, const double* part, void* out, ma_stream_t stream) {
  if (!y || !part || !out) return MA_ERR_INVALID_ARG;
  int64_t tiles = 0;
  const int rc = check_tiles(M, K, C, &tiles);
  if (rc != MA_OK) return rc;
  if (!aligned16(y) || (reinterpret_cast<uintptr_t>(out) & 7)) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(gln_apply_bf16_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, y, K, C, tile_rows(C),
            part, (int)tiles, reinterpret_cast<uint16_t*>(out));
  return MA_OK;
}

extern "C" int ma_tasnet_decode_f32(const float* score, const float* mixture_w, int64_t M, int64_t K, int32_t C, int32_t N,
                                    const float* basis, int32_t L, int32_t overlap, float* out, ma_stream_t stream) {
  if (!score || !mixture_w || !basis || !out || M < 1 || K < 1 || C < 1 || N < 1 || L < 2) return MA_ERR_INVALID_ARG;
  if (overlap != MA_TASNET_OVERLAP_PAIRED && overlap != MA_TASNET_OVERLAP_TRUE) return MA_ERR_INVALID_ARG;
  const size_t lds = (size_t)(kTnThreads / 64) * kDecFrames * N * sizeof(float);
  if ((L & 1) || L > 64 || N % 64 != 0 || lds > 60 * 1024 || M * C > 65535 || M * K > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  const int64_t waves = (K + 1 + kDecSeg - 1) / kDecSeg, blocks = (waves + kTnThreads / 64 - 1) / (kTnThreads / 64);
  MA_LAUNCH(tasnet_decode_kernel, dim3((unsigned)blocks, (unsigned)(M * C)), dim3(kTnThreads), lds, (hipStream_t)stream, score, mixture_w,
            K, C, N, basis, L, overlap == MA_TASNET_OVERLAP_TRUE ? 1 : 0, out);
  return MA_OK;
}

extern "C" int ma_si_snr_pairwise(const float* source, const float* estimate, const int64_t* lengths, int64_t B, int32_t C, int64_t T,
                                  double* out, ma_stream_t stream) {
  if (!source || !estimate || !lengths || !out || B < 1 || C < 1 || T < 1) return MA_ERR_INVALID_ARG;
  if (C > 8 || B * C * C > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(si_snr_pairwise_kernel, dim3((unsigned)(B * C * C)), dim3(kTnThreads), 0, (hipStream_t)stream, source, estimate, lengths, C, T,
            out);
  return MA_OK;
}
