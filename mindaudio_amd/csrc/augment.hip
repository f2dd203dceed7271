// Time-domain augmentation chain of ECAPA training-data generation (mindaudio/data/augment.py as driven by
// examples/ECAPA-TDNN/spec_augment.py): row statistics, the circular FIR of drop_freq, the FFT convolution of reverberate, the babble
// sum, the amplitude-scaled mixes of add_noise / add_babble and the interval fill of drop_chunk.  Contract: include/mindaudio_amd.h.
// Random decisions are the host's (the reference's np.random / random call order); the kernels take them as small device arrays.
// Every amplitude a later step needs stays on the device in `double stats[rows][4]`; no launcher synchronises or allocates.
// Sums: float64 accumulation per thread over a fixed stride, then a fixed shuffle / LDS tree - the same bits every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "launch.h"

namespace ma {

// sum over the workgroup (blockDim.x a multiple of 64, at most 1024), the same value in every thread; sh: 16 entries
template <typename T>
__device__ __forceinline__ T aug_block_sum(T v, T* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int nw = blockDim.x >> 6;
  __syncthreads();  // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = (T)0;
  for (int i = 0; i < nw; ++i) t += sh[i];
  return t;
}

// ---- row statistics: one workgroup of 1024 lanes per row (48 000 samples: 47 coalesced loads per lane) -------------------------
__global__ __launch_bounds__(1024) void aug_row_stats_kernel(const float* __restrict__ x, int64_t ldx, int64_t n,
                                                             double* __restrict__ stats) {
  __shared__ double sh[16];
  __shared__ float shm[16];
  const float* xr = x + (int64_t)blockIdx.x * ldx;
  double sa = 0.0, sq = 0.0;
  float mx = 0.0f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float v = xr[i];
    const float a = fabsf(v);
    sa += (double)a;
    sq += (double)v * (double)v;
    mx = fmaxf(mx, a);
  }
  sa = aug_block_sum(sa, sh);
  sq = aug_block_sum(sq, sh);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_down(mx, o, 64));
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = shm[0];
    for (int i = 1; i < 16; ++i) m = fmaxf(m, shm[i]);
    double* st = stats + (int64_t)blockIdx.x * 4;
    st[0] = sa;
    st[1] = sq;
    st[2] = (double)m;
    st[3] = 0.0;
  }
}

// ---- circular FIR ------------------------------------------------------------------------------------------------------------------
// A workgroup writes a tile of 2048 outputs of one row: the tile and a halo of K8 = roundup(K, 8) samples in front of it (wrapped at
// the seam of the row) sit in LDS, the taps (zero-padded to K8) too.  A lane owns 8 consecutive outputs and walks the taps in blocks
// of 8 with a 16-sample register window: 8 window loads + 8 tap broadcasts per 64 multiply-adds.  Lane l reads LDS word 8 l + c; one
// padding word per 32 spreads a half-wave's 32 reads over the 32 banks (8 (l % 4) + l / 4 + c).
constexpr int kFirTile = 2048;
__device__ __forceinline__ int fir_pad(int i) { return i + (i >> 5); }
constexpr int fir_lds_floats(int k8) { return k8 + (kFirTile + k8) + ((kFirTile + k8) >> 5) + 1; }

__global__ __launch_bounds__(256) void aug_circular_fir_kernel(const float* __restrict__ x, int64_t ldx, int64_t n,
                                                               const float* __restrict__ h, int K, int K8, float* __restrict__ out,
                                                               int64_t ldo, int64_t n_out) {
  extern __shared__ __attribute__((aligned(16))) float fir_smem[];
  float* taps = fir_smem;       // [K8]
  float* s = fir_smem + K8;     // [fir_pad(kFirTile + K8)]: s[i] = x[(n0 - K8 + i) mod n]
  const int tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * kFirTile;
  const float* xr = x + (int64_t)blockIdx.y * ldx;
  float* orow = out + (int64_t)blockIdx.y * ldo;
  for (int k = tid; k < K8; k += 256) taps[k] = k < K ? h[k] : 0.0f;
  const int total = kFirTile + K8;
  {
    int64_t g = (n0 - K8 + tid) % n;  // (C++ remainder: sign of the dividend)
    if (g < 0) g += n;
    const int64_t step = 256 % n;
    for (int i = tid; i < total; i += 256) {
      s[fir_pad(i)] = xr[g];
      g += step;
      if (g >= n) g -= n;
    }
  }
  __syncthreads();
  float y[8], v[16];
  const int p = K8 + 8 * tid;  // LDS index of this lane's first output at tap 0
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = 0.0f;
#pragma unroll
  for (int m = 0; m < 8; ++m) v[8 + m] = s[fir_pad(p + m)];
  for (int kb = 0; kb < K8; kb += 8) {  // v[m] = s[p - kb - 8 + m]
#pragma unroll
    for (int m = 0; m < 8; ++m) v[m] = s[fir_pad(p - kb - 8 + m)];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const float hk = taps[kb + kk];
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = fmaf(hk, v[8 + j - kk], y[j]);
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) v[8 + m] = v[m];
  }
  const int64_t i0 = n0 + 8 * tid;
  if (i0 + 8 <= n && i0 + 8 <= n_out && ((reinterpret_cast<uintptr_t>(orow + i0) & 15) == 0)) {
    float4* o4 = reinterpret_cast<float4*>(orow + i0);
    o4[0] = make_float4(y[0], y[1], y[2], y[3]);
    o4[1] = make_float4(y[4], y[5], y[6], y[7]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i0 + j < n_out) orow[i0 + j] = (i0 + j < n) ? y[j] : 0.0f;
  }
}

// ---- FFT convolution ---------------------------------------------------------------------------------------------------------------
// Transform p < pairs holds rows 2p (real part) and 2p + 1 (imaginary part) zero-padded to L; transform `pairs` holds the filter.
__global__ __launch_bounds__(256) void aug_pack_pairs_kernel(const float* __restrict__ x, int64_t ldx, int64_t rows, int64_t n,
                                                             const float* __restrict__ h, int64_t K, int64_t L,
                                                             float2* __restrict__ A) {
  const int64_t p = blockIdx.y, pairs = (rows + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= L) return;
  float re = 0.0f, im = 0.0f;
  if (p < pairs) {
    if (i < n) {
      re = x[2 * p * ldx + i];
      if (2 * p + 1 < rows) im = x[(2 * p + 1) * ldx + i];
    }
  } else if (i < K) {
    re = h[i];
  }
  A[p * L + i] = make_float2(re, im);
}

// A[p] *= H for every pair p (the filter is real, so the two packed rows stay separate: conv(x1 + i x2, h) = conv(x1, h) + i conv(x2, h))
__global__ __launch_bounds__(256) void aug_spectrum_mul_kernel(float2* __restrict__ A, const float2* __restrict__ H, int64_t L) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= L) return;
  const float2 a = A[(int64_t)blockIdx.y * L + i], b = H[i];
  float2 c;
  c.x = a.x * b.x - a.y * b.y;
  c.y = a.x * b.y + a.y * b.x;
  A[(int64_t)blockIdx.y * L + i] = c;
}

// y[r][i] = (lin[m] + lin[m + n] [m < K - 1]) / L, m = (i + rot) mod n: the fold of the linear convolution's tail, the rotation, the
// 1 / L of the unscaled inverse transform and the block's share of sum |y| in the pass that writes y.  1024 columns per workgroup.
__global__ __launch_bounds__(256) void aug_fold_out_kernel(const float2* __restrict__ C, int64_t L, int64_t n, int64_t K, int64_t rot,
                                                           float inv_l, float* __restrict__ out, int64_t ldo, int64_t n_out,
                                                           double* __restrict__ partial, int nb) {
  __shared__ double sh[16];
  const int64_t r = blockIdx.y;
  const float* c = reinterpret_cast<const float*>(C + (r >> 1) * L) + (r & 1);
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
    float v = 0.0f;
    if (i < n) {
      int64_t m = i + rot;
      if (m >= n) m -= n;
      v = c[2 * m];
      if (m < K - 1) v += c[2 * (m + n)];
      v *= inv_l;
      acc += (double)fabsf(v);
    }
    if (i < n_out) out[r * ldo + i] = v;
  }
  acc = aug_block_sum(acc, sh);
  if (threadIdx.x == 0) partial[r * nb + blockIdx.x] = acc;
}

// out[r] *= amp(x) / (amp(y) + 1e-14): sum |y| from the partials of aug_fold_out_kernel, summed in a fixed order by every workgroup
__global__ __launch_bounds__(256) void aug_rescale_avg_kernel(float* __restrict__ out, int64_t ldo, int64_t n, int64_t n_out,
                                                              const double* __restrict__ partial, int nb,
                                                              const double* __restrict__ stats_x) {
  __shared__ double sh[16];
  const int64_t r = blockIdx.y;
  double sy = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) sy += partial[r * nb + b];
  sy = aug_block_sum(sy, sh);
  const double ax = stats_x[r * 4] / (double)n, ay = sy / (double)n;
  const float g = (float)(ax / (ay + 1e-14));
  const int64_t lim = n < n_out ? n : n_out;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
    if (i < lim) out[r * ldo + i] *= g;
  }
}

// ---- babble sum, mix, interval fill -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aug_babble_sum_kernel(const float* __restrict__ x, int64_t ldx, int rows, int64_t n, int speakers,
                                                             float* __restrict__ out, int64_t ldo) {
  const int r = blockIdx.y;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
    if (i >= n) continue;
    float acc = 0.0f;
    for (int k = 1; k <= speakers; ++k) {
      int q = (r - k) % rows;
      if (q < 0) q += rows;
      const float v = x[(int64_t)q * ldx + i];
      acc = k == 1 ? v : acc + v;
    }
    out[(int64_t)r * ldo + i] = acc;
  }
}

__global__ __launch_bounds__(256) void aug_mix_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, const float* __restrict__ noise,
                                                      int64_t ld_noise, int mode, float gain, const double* __restrict__ params,
                                                      const double* __restrict__ stats_x, const double* __restrict__ stats_noise,
                                                      float* __restrict__ out, int64_t ldo, int64_t n_out) {
  const int64_t r = blockIdx.y;
  float a = 1.0f, s = 0.0f;
  if (mode == MA_AUG_MIX_NOISE) {
    s = (float)((double)gain * sqrt(stats_x[r * 4 + 1] / (double)n));
  } else if (mode == MA_AUG_MIX_BABBLE) {
    const double f = params[r * 4], len = params[r * 4 + 1], blen = params[r * 4 + 2];
    a = (float)(1.0 - f);
    s = (float)(f * (stats_x[r * 4] / len) / (stats_noise[r * 4] / blen + 1e-14));
  } else if (mode == MA_AUG_MIX_UNIT_AVG) {
    a = (float)((double)gain / (stats_x[r * 4] / params[r * 4] + 1e-14));
  } else if (mode == MA_AUG_MIX_UNIT_PEAK) {
    a = (float)((double)gain / (stats_x[r * 4 + 2] + 1e-14));
  } else {
    a = (float)((double)gain / (sqrt(stats_x[r * 4 + 1] / (double)n) + 1e-8));
  }
  const bool with_noise = mode == MA_AUG_MIX_NOISE || mode == MA_AUG_MIX_BABBLE;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
    if (i >= n_out) continue;
    float v = 0.0f;
    if (i < n) {
      const float xv = x[r * ldx + i];
      v = with_noise ? fmaf(s, noise[r * ld_noise + i], a * xv) : a * xv;
    }
    out[r * ldo + i] = v;
  }
}

__global__ __launch_bounds__(256) void aug_drop_chunks_kernel(const float* __restrict__ x, int64_t ldx, int64_t n,
                                                              const int32_t* __restrict__ intervals, int n_max,
                                                              const float* __restrict__ fill, const int32_t* __restrict__ fill_off,
                                                              float noise_factor, const double* __restrict__ stats,
                                                              const double* __restrict__ lens, float* __restrict__ out, int64_t ldo,
                                                              int64_t n_out) {
  __shared__ int32_t iv[256][2];
  __shared__ int32_t off[256];
  const int64_t r = blockIdx.y;
  for (int j = threadIdx.x; j < n_max; j += 256) {
    iv[j][0] = intervals[(r * n_max + j) * 2];
    iv[j][1] = intervals[(r * n_max + j) * 2 + 1];
    off[j] = fill ? fill_off[r * n_max + j] : 0;
  }
  __syncthreads();
  float m = 0.0f;
  if (fill) m = (float)(2.0 * (double)noise_factor * (stats[r * 4] / lens[r]));
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + u * 256 + threadIdx.x;
    if (i >= n_out) continue;
    float v = 0.0f;
    if (i < n) {
      int hit = -1;
      for (int j = 0; j < n_max; ++j)
        if (i >= iv[j][0] && i < iv[j][1]) hit = j;
      if (hit < 0) {
        v = x[r * ldx + i];
      } else if (fill) {
        const float uu = fill[(int64_t)off[hit] + (i - iv[hit][0])];
        v = 2.0f * m * uu - m;
      }
    }
    out[r * ldo + i] = v;
  }
}

static bool aug_rows_ok(const void* x, int64_t ld, int64_t rows, int64_t n) {
  return x && rows >= 1 && rows <= 65535 && n >= 1 && ld >= n;
}

}  // namespace ma

using namespace ma;

extern "C" int ma_aug_row_stats_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, double* stats, ma_stream_t stream) {
  if (!aug_rows_ok(x, ldx, rows, n) || !stats) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(aug_row_stats_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, x, ldx, n, stats);
  return MA_OK;
}

extern "C" int ma_aug_circular_fir_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, const float* h, int32_t K, float* out,
                                       int64_t ldo, int64_t n_out, ma_stream_t stream) {
  if (!aug_rows_ok(x, ldx, rows, n) || !h || !out || K < 1 || K > 255 || n_out < 1 || ldo < n_out || out == x)
    return MA_ERR_INVALID_ARG;
  const int K8 = (K + 7) & ~7;
  const dim3 grid((unsigned)((n_out + kFirTile - 1) / kFirTile), (unsigned)rows);
  MA_LAUNCH(aug_circular_fir_kernel, grid, dim3(256), fir_lds_floats(K8) * sizeof(float), (hipStream_t)stream, x, ldx, n, h, (int)K, K8,
            out, ldo, n_out);
  return MA_OK;
}

extern "C" int64_t ma_aug_fft_conv_length(int64_t n, int64_t K) {
  if (n < 1 || K < 1 || K > n) return MA_ERR_INVALID_ARG;
  int64_t L = 2048;  // the shortest transform ma_fft_pow2_c32 runs
  while (L < n + K - 1) L <<= 1;
  return L > ((int64_t)1 << 26) ? MA_ERR_UNSUPPORTED : L;
}

static int64_t aug_fold_blocks(int64_t n, int64_t n_out) { return ((n > n_out ? n : n_out) + 1023) / 1024; }

extern "C" int64_t ma_aug_fft_conv_workspace_bytes(int64_t rows, int64_t n, int64_t K) {
  const int64_t L = ma_aug_fft_conv_length(n, K);
  if (L < 0) return L;
  if (rows < 1 || rows > 65535) return MA_ERR_INVALID_ARG;
  /* two buffers of pairs + 1 transforms, and the partial sums of |y| for outputs of up to 2 n columns */
  return 2 * ((rows + 1) / 2 + 1) * L * 8 + rows * aug_fold_blocks(n, 2 * n) * 8;
}

extern "C" int ma_aug_fft_conv_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, const float* h, int64_t K, int64_t rot,
                                   const double* stats_x, float* out, int64_t ldo, int64_t n_out, void* workspace,
                                   int64_t workspace_bytes, ma_stream_t stream) {
  if (!aug_rows_ok(x, ldx, rows, n) || !h || !out || !workspace || n_out < 1 || n_out > 2 * n || ldo < n_out || rot < 0 ||
      rot > K)
    return MA_ERR_INVALID_ARG;
  const int64_t L = ma_aug_fft_conv_length(n, K);
  if (L < 0) return (int)L;
  if (workspace_bytes < ma_aug_fft_conv_workspace_bytes(rows, n, K)) return MA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t pairs = (rows + 1) / 2;
  float2* A = reinterpret_cast<float2*>(workspace);
  float2* T = A + (pairs + 1) * L;
  double* partial = reinterpret_cast<double*>(T + (pairs + 1) * L);
  const unsigned lb = (unsigned)((L + 255) / 256);
  MA_LAUNCH(aug_pack_pairs_kernel, dim3(lb, (unsigned)(pairs + 1)), dim3(256), 0, st, x, ldx, rows, n, h, K, L, A);
  void* res = nullptr;
  int rc = ma_fft_pow2_c32(A, T, pairs + 1, L, 0, &res, stream);
  if (rc != MA_OK) return rc;
  float2* F = reinterpret_cast<float2*>(res);
  float2* other = F == A ? T : A;
  MA_LAUNCH(aug_spectrum_mul_kernel, dim3(lb, (unsigned)pairs), dim3(256), 0, st, F, F + pairs * L, L);
  rc = ma_fft_pow2_c32(F, other, pairs, L, 1, &res, stream);
  if (rc != MA_OK) return rc;
  const int nb = (int)aug_fold_blocks(n, n_out);
  const dim3 grid((unsigned)nb, (unsigned)rows);
  MA_LAUNCH(aug_fold_out_kernel, grid, dim3(256), 0, st, reinterpret_cast<const float2*>(res), L, n, K, rot, 1.0f / (float)L, out, ldo,
            n_out, partial, nb);
  if (stats_x) MA_LAUNCH(aug_rescale_avg_kernel, grid, dim3(256), 0, st, out, ldo, n, n_out, partial, nb, stats_x);
  return MA_OK;
}

extern "C" int ma_aug_babble_sum_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, int32_t speakers, float* out, int64_t ldo,
                                     ma_stream_t stream) {
  if (!aug_rows_ok(x, ldx, rows, n) || !out || ldo < n || speakers < 1 || out == x) return MA_ERR_INVALID_ARG;
  const dim3 grid((unsigned)((n + 1023) / 1024), (unsigned)rows);
  MA_LAUNCH(aug_babble_sum_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, (int)rows, n, (int)speakers, out, ldo);
  return MA_OK;
}

extern "C" int ma_aug_mix_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, const float* noise, int64_t ld_noise, int32_t mode,
                              float gain, const double* params, const double* stats_x, const double* stats_noise, float* out,
                              int64_t ldo, int64_t n_out, ma_stream_t stream) {
  if (!aug_rows_ok(x, ldx, rows, n) || !out || n_out < 1 || ldo < n_out || !stats_x) return MA_ERR_INVALID_ARG;
  if (mode == MA_AUG_MIX_NOISE) {
    if (!noise || (ld_noise != 0 && ld_noise < n)) return MA_ERR_INVALID_ARG;
  } else if (mode == MA_AUG_MIX_BABBLE) {
    if (!noise || !params || !stats_noise || (ld_noise != 0 && ld_noise < n)) return MA_ERR_INVALID_ARG;
  } else if (mode == MA_AUG_MIX_UNIT_AVG) {
    if (!params) return MA_ERR_INVALID_ARG;
  } else if (mode != MA_AUG_MIX_UNIT_PEAK && mode != MA_AUG_MIX_UNIT_RMS) {
    return MA_ERR_INVALID_ARG;
  }
  const dim3 grid((unsigned)((n_out + 1023) / 1024), (unsigned)rows);
  MA_LAUNCH(aug_mix_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, n, noise, ld_noise, (int)mode, gain, params, stats_x,
            stats_noise, out, ldo, n_out);
  return MA_OK;
}

extern "C" int ma_aug_drop_chunks_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, const int32_t* intervals, int32_t n_max,
                                      const float* fill, const int32_t* fill_off, float noise_factor, const double* stats,
                                      const double* lens, float* out, int64_t ldo, int64_t n_out, ma_stream_t stream) {
  if (!aug_rows_ok(x, ldx, rows, n) || !out || n_out < 1 || ldo < n_out || n_max < 0 || n_max > 256 || (n_max > 0 && !intervals) ||
      out == x || n > 0x7fffffff)
    return MA_ERR_INVALID_ARG;
  if (fill && (!fill_off || !stats || !lens)) return MA_ERR_INVALID_ARG;
  const dim3 grid((unsigned)((n_out + 1023) / 1024), (unsigned)rows);
  MA_LAUNCH(aug_drop_chunks_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, n, intervals, (int)n_max, fill, fill_off,
            noise_factor, stats, lens, out, ldo, n_out);
  return MA_OK;
}
