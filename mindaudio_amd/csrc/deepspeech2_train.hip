// DeepSpeech2's convolution front end (MaskConv) in TRAINING mode: what sits between the library's products when conv1, conv2 and both
// BatchNorm2d are trained (models/deepspeech2_train.py, frontend="trained").  Contract: include/mindaudio_amd.h.
//
//   forward   ds2_conv1_raw_kernel   ds2_conv1_kernel (deepspeech2.hip) without its epilogue: the float32 accumulators y1 (T1, B, F1, 32)
//                                    and the workgroup's (sum | sum of squares) per channel
//             ds2_stats_kernel       the same partials of any channel-last float32 array (conv2's raw output, channel = column mod 32)
//             ds2_bn_finalize_kernel partials -> mean, rstd of the biased variance, the biased variance; the moving statistics are READ
//                                    from one pair of vectors and WRITTEN to another (the trainer commits them after its overflow check)
//             ds2_bn_tanh_fwd_kernel a = tanh(fma(gamma, (y - mean) * rstd, beta)) as bf16 into a strided image
//   backward  ds2_bn_tanh_bwd1/2     BatchNorm + tanh backward in two passes with a join between them (one pair serves both stages)
//             ds2_conv1_dw_kernel    conv1's weight gradient, the mirror of ds2_conv1_kernel, and its join
//             ds2_commit_kernel      dst = src unless the step's overflow flag is set
// conv2's weight and input gradients are ma_gemm_tn_bf16_f32 / ma_conv1d_taps_bf16 calls of the caller.
//
// Sums.  Every statistic is accumulated in DOUBLE by a thread, joined in double over the workgroup's threads in a fixed order, stored as
// a double partial per workgroup and joined in double in partial order (train_kernels.hip, bn_finalize_kernel, has the reason: the
// variance is E[y^2] - mean^2).  No atomics anywhere: two runs give the same bits.
//
// ds2_conv1_dw_kernel.  dW1[c, kf, kt] = sum over (b, f1, t1) of dz1[t1, b, f1, c] * x[b, 2 f1 + kf - 20, 2 t1 + kt - 5].  A workgroup
// walks `fpw` consecutive frames (t1, b); per frame it stages the input patch ((F + 40) x 11, zero padded, as the forward) and the
// frame's dz1 (F1, 32) in LDS.  With the patch stored row-major the input of tap = kf * 11 + kt at output frequency f1 is
// patch[22 f1 + tap]: thread (cq = tid & 7, g = tid >> 3) owns the channels 4 cq .. 4 cq + 3 of the taps g, g + 32, .. (15 slots, 60
// accumulators); per f1 one 16-byte LDS read of its four dz1 and one 4-byte read per tap feed 4 FMAs each.  A wave's 4-byte reads:
// lanes with one g share an address (broadcast), the 4 g of a 32-lane group are consecutive words - no bank conflict; the 16-byte
// reads of a 16-lane group are 128 contiguous bytes.
// Accumulation: the LONGEST FLOAT32 CHAIN is fpw * F1 fused multiply-adds per accumulator (fpw = ceil(B T1 / 1024) unless the caller
// sets it: 40 * 81 = 3240 at B = 64, T = 1250, F = 161); the <= 1024 workgroup partials are then added in double in partial order and
// rounded once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kFeC = 32, kFeKf = 41, kFeKt = 11, kFeTaps = kFeKf * kFeKt;
constexpr int kFeMaxF = 256, kFeNi = 4, kFeFramesPerWg = 8;
constexpr int kFeConvLds = kFeTaps * kFeC * 4 + (kFeMaxF + 40) * kFeKt * 4;
constexpr int kFeDwSlots = (kFeTaps + 31) / 32;  // 15 taps per thread
constexpr int kFeMaxParts = 1024;

// The workgroup's per-channel sums from per-thread sums: thread (cq = tid & 7, g = tid >> 3) holds a[k], b[k] of channel 4 cq + k.
// red: 256 * 8 doubles of LDS that nothing else uses any more.  out[0..31] = sum a, out[32..63] = sum b, added over g = 0 .. 31 in order.
__device__ __forceinline__ void wg_join_channels(const double (&a)[4], const double (&b)[4], double* red, double* out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    red[tid * 8 + k] = a[k];
    red[tid * 8 + 4 + k] = b[k];
  }
  __syncthreads();
  if (tid < 64) {
    const int c = tid & 31, which = tid >> 5;
    double s = 0.0;
    for (int g = 0; g < 32; ++g) s += red[(g * 8 + (c >> 2)) * 8 + which * 4 + (c & 3)];
    out[tid] = s;
  }
}

// ds2_conv1_kernel's staging and tap loop (same order of the fmaf chain, hence the same accumulators); the epilogue stores them raw.
__global__ __launch_bounds__(256) void ds2_conv1_raw_kernel(const float* __restrict__ x, int F, int T, int B, int F1, int T1,
                                                            const float* __restrict__ wt, float* __restrict__ y1,
                                                            double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = reinterpret_cast<float*>(smem);  // (451, 32)
  float* patch = wl + kFeTaps * kFeC;          // (F + 40, 11): input rows f - 20, columns 2 t1 - 5 + kt
  const int tid = threadIdx.x, cq = tid & 7, g = tid >> 3;
  const int b = blockIdx.y;
  for (int i = tid; i < kFeTaps * kFeC; i += 256) wl[i] = wt[i];
  const int prow = F + 40;
  const float* xb = x + (int64_t)b * F * T;
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < kFeFramesPerWg; ++it) {
    const int t1 = blockIdx.x * kFeFramesPerWg + it;
    if (t1 >= T1) break;  // (uniform over the workgroup)
    __syncthreads();
    for (int i = tid; i < prow * kFeKt; i += 256) {
      const int r = i / kFeKt, kt = i - r * kFeKt;
      const int f = r - 20, t = 2 * t1 - 5 + kt;
      patch[i] = (f >= 0 && f < F && t >= 0 && t < T) ? xb[(int64_t)f * T + t] : 0.0f;
    }
    __syncthreads();
    f32x4 acc[kFeNi];
#pragma unroll
    for (int i = 0; i < kFeNi; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kf = 0; kf < kFeKf; ++kf)
      for (int kt = 0; kt < kFeKt; ++kt) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wl + (kf * kFeKt + kt) * kFeC + 4 * cq);
#pragma unroll
        for (int i = 0; i < kFeNi; ++i) {
          const int f1 = g + 32 * i;
          if (f1 < F1) {
            const float xv = patch[(2 * f1 + kf) * kFeKt + kt];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(w[c], xv, acc[i][c]);
          }
        }
      }
    float* o = y1 + ((int64_t)t1 * B + b) * F1 * kFeC + 4 * cq;
#pragma unroll
    for (int i = 0; i < kFeNi; ++i) {
      const int f1 = g + 32 * i;
      if (f1 < F1) {
        *reinterpret_cast<f32x4*>(o + (int64_t)f1 * kFeC) = acc[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          s1[c] += (double)acc[i][c];
          s2[c] += (double)acc[i][c] * (double)acc[i][c];
        }
      }
    }
  }
  __syncthreads();  // the weights and the patch have been read: their LDS becomes the join's
  wg_join_channels(s1, s2, reinterpret_cast<double*>(smem), part + (int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * 64);
}
MA_LDS_ATTR(ds2_conv1_raw_kernel, kFeConvLds);

// y: n32 runs of 32 channels; workgroup w takes the runs [w * per, (w + 1) * per)
__global__ __launch_bounds__(256) void ds2_stats_kernel(const float* __restrict__ y, int64_t n32, int64_t per, double* __restrict__ part) {
  __shared__ double red[256 * 8];
  const int tid = threadIdx.x, cq = tid & 7, g = tid >> 3;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < n32 ? lo + per : n32;
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = lo + g; r < hi; r += 32) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + r * kFeC + 4 * cq);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s1[c] += (double)v[c];
      s2[c] += (double)v[c] * (double)v[c];
    }
  }
  wg_join_channels(s1, s2, red, part + (int64_t)blockIdx.x * 64);
}

// part (nparts, 64) doubles -> sums[64], four strided chains joined in order (one workgroup of 256 threads); valid for tid < 64
__device__ __forceinline__ double join_parts64(const double* __restrict__ part, int nparts, double (*red)[64]) {
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  double s = 0.0;
  for (int p = grp; p < nparts; p += 4) s += part[(int64_t)p * 64 + col];
  red[grp][col] = s;
  __syncthreads();
  return red[0][col] + red[1][col] + red[2][col] + red[3][col];
}

// stats = (mean | rstd | biased variance); moving_out = (1 - momentum) * moving_in + momentum * (mean, unbiased variance)
__global__ __launch_bounds__(256) void ds2_bn_finalize_kernel(const double* __restrict__ part, int nparts, double count, float eps,
                                                              float momentum, const float* __restrict__ mean_in,
                                                              const float* __restrict__ var_in, float* __restrict__ mean_out,
                                                              float* __restrict__ var_out, float* __restrict__ stats) {
  __shared__ double red[4][64];
  __shared__ double tot[64];
  const double s = join_parts64(part, nparts, red);
  if (threadIdx.x < 64) tot[threadIdx.x] = s;
  __syncthreads();
  const int c = threadIdx.x;
  if (c >= kFeC) return;
  const double mean = tot[c] / count;
  double var = tot[kFeC + c] / count - mean * mean;
  var = var < 0.0 ? 0.0 : var;  // (a NaN stays a NaN)
  stats[c] = (float)mean;
  stats[kFeC + c] = (float)(1.0 / sqrt(var + (double)eps));
  stats[2 * kFeC + c] = (float)var;
  if (mean_out) {
    const double m = (double)momentum, unbiased = var * (count / fmax(count - 1.0, 1.0));
    mean_out[c] = (float)((1.0 - m) * (double)mean_in[c] + m * mean);
    var_out[c] = (float)((1.0 - m) * (double)var_in[c] + m * unbiased);
  }
}

__device__ __forceinline__ float bn_tanh(float y, float mean, float rstd, float gamma, float beta, float& xhat) {
  xhat = (y - mean) * rstd;
  return tanhf(fmaf(gamma, xhat, beta));
}
// dn = dout (1 - a^2) with a recomputed; ONE spelling for both backward passes, so that they see the same bits
__device__ __forceinline__ float bn_tanh_dn(float y, float d, float mean, float rstd, float gamma, float beta, float& xhat) {
  const float a = bn_tanh(y, mean, rstd, gamma, beta, xhat);
  return d * fmaf(-a, a, 1.0f);
}

// out[row * ldo + col] = bf16(tanh(gamma (y - mean) rstd + beta)), y (rows, cols) contiguous, channel = col & 31
__global__ __launch_bounds__(256) void ds2_bn_tanh_fwd_kernel(const float* __restrict__ y, int64_t rows, int cols,
                                                              const float* __restrict__ stats, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, uint16_t* __restrict__ out, int64_t ldo) {
  const int q = cols >> 2;
  const int64_t n = rows * q;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / q;
    const int col = (int)(i - row * q) * 4, c = col & 31;
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + i * 4);
    float a[4], xh;
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = bn_tanh(v[k], stats[c + k], stats[kFeC + c + k], gamma[c + k], beta[c + k], xh);
    uint2 w;
    w.x = (uint32_t)f2bf(a[0]) | ((uint32_t)f2bf(a[1]) << 16);
    w.y = (uint32_t)f2bf(a[2]) | ((uint32_t)f2bf(a[3]) << 16);
    *reinterpret_cast<uint2*>(out + row * ldo + col) = w;
  }
}

// pass 1: dn = dout (1 - a^2); the workgroup's (sum dn | sum dn xhat) per channel.  y (rows, nf * 32) contiguous, dout row stride ldd;
// workgroup w takes the runs [w * per, (w + 1) * per) of the rows * nf runs of 32 channels.
__global__ __launch_bounds__(256) void ds2_bn_tanh_bwd1_kernel(const float* __restrict__ y, const float* __restrict__ dout, int64_t ldd,
                                                               int64_t n32, int nf, int64_t per, const float* __restrict__ stats,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               double* __restrict__ part) {
  __shared__ double red[256 * 8];
  const int tid = threadIdx.x, cq = tid & 7, g = tid >> 3;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < n32 ? lo + per : n32;
  float mean[4], rstd[4], ga[4], be[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    mean[k] = stats[4 * cq + k];
    rstd[k] = stats[kFeC + 4 * cq + k];
    ga[k] = gamma[4 * cq + k];
    be[k] = beta[4 * cq + k];
  }
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = lo + g; r < hi; r += 32) {
    const int64_t row = r / nf;
    const int f = (int)(r - row * nf);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + r * kFeC + 4 * cq);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + row * ldd + f * kFeC + 4 * cq);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float xh;
      const float dn = bn_tanh_dn(v[k], d[k], mean[k], rstd[k], ga[k], be[k], xh);
      s1[k] += (double)dn;
      s2[k] += (double)dn * (double)xh;
    }
  }
  wg_join_channels(s1, s2, red, part + (int64_t)blockIdx.x * 64);
}

// bsum = (d_beta | d_gamma | mean dn | mean dn xhat); d_gamma / d_beta (optional) receive the parameter gradients too
__global__ __launch_bounds__(256) void ds2_bn_bwd_join_kernel(const double* __restrict__ part, int nparts, double count,
                                                              float* __restrict__ bsum, float* __restrict__ d_gamma,
                                                              float* __restrict__ d_beta) {
  __shared__ double red[4][64];
  const double s = join_parts64(part, nparts, red);
  const int col = threadIdx.x;
  if (col >= 64) return;
  bsum[col] = (float)s;
  bsum[64 + col] = (float)(s / count);
  if (col < kFeC && d_beta) d_beta[col] = (float)s;
  if (col >= kFeC && d_gamma) d_gamma[col - kFeC] = (float)s;
}

// pass 2: dz = gamma rstd (dn - mean(dn) - xhat mean(dn xhat)) -> out[row * ldo + col], float32 or bf16
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void ds2_bn_tanh_bwd2_kernel(const float* __restrict__ y, const float* __restrict__ dout, int64_t ldd,
                                                               int64_t rows, int cols, const float* __restrict__ stats,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ bsum, void* __restrict__ out, int64_t ldo) {
  const int q = cols >> 2;
  const int64_t n = rows * q;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / q;
    const int col = (int)(i - row * q) * 4, c = col & 31;
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + i * 4);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + row * ldd + col);
    float dz[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float xh;
      const float dn = bn_tanh_dn(v[k], d[k], stats[c + k], stats[kFeC + c + k], gamma[c + k], beta[c + k], xh);
      dz[k] = gamma[c + k] * stats[kFeC + c + k] * (dn - bsum[64 + c + k] - xh * bsum[96 + c + k]);
    }
    if constexpr (OUT_BF16) {
      uint2 w;
      w.x = (uint32_t)f2bf(dz[0]) | ((uint32_t)f2bf(dz[1]) << 16);
      w.y = (uint32_t)f2bf(dz[2]) | ((uint32_t)f2bf(dz[3]) << 16);
      *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out) + row * ldo + col) = w;
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + row * ldo + col) = f32x4{dz[0], dz[1], dz[2], dz[3]};
    }
  }
}

__host__ __device__ constexpr int fe_dw_patch_words(int F) { return ((F + 40) * kFeKt + 32 + 3) / 4 * 4; }  // + the last slot's overrun

__global__ __launch_bounds__(256) void ds2_conv1_dw_kernel(const float* __restrict__ x, int F, int T, int B, int F1, int T1,
                                                           const float* __restrict__ dz1, int fpw, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* patch = reinterpret_cast<float*>(smem);  // (F + 40, 11) and 32 zero words: slot 14 of a thread with g >= 3 reads past tap 450
  const int pw = fe_dw_patch_words(F), prow = F + 40;
  float* dzl = patch + pw;                        // (F1, 32)
  const int tid = threadIdx.x, cq = tid & 7, g = tid >> 3;
  for (int i = prow * kFeKt + tid; i < pw; i += 256) patch[i] = 0.0f;
  f32x4 acc[kFeDwSlots];
#pragma unroll
  for (int i = 0; i < kFeDwSlots; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t frames = (int64_t)B * T1;
  for (int it = 0; it < fpw; ++it) {
    const int64_t fr = (int64_t)blockIdx.x * fpw + it;  // = t1 * B + b, the row order of dz1
    if (fr >= frames) break;                            // (uniform over the workgroup)
    const int t1 = (int)(fr / B), b = (int)(fr - (int64_t)t1 * B);
    const float* xb = x + (int64_t)b * F * T;
    __syncthreads();  // the previous frame has been read
    for (int i = tid; i < prow * kFeKt; i += 256) {
      const int r = i / kFeKt, kt = i - r * kFeKt;
      const int f = r - 20, t = 2 * t1 - 5 + kt;
      patch[i] = (f >= 0 && f < F && t >= 0 && t < T) ? xb[(int64_t)f * T + t] : 0.0f;
    }
    const f32x4* src = reinterpret_cast<const f32x4*>(dz1 + fr * F1 * kFeC);
    for (int i = tid; i < F1 * (kFeC / 4); i += 256) reinterpret_cast<f32x4*>(dzl)[i] = src[i];
    __syncthreads();
    for (int f1 = 0; f1 < F1; ++f1) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(dzl + f1 * kFeC + 4 * cq);
      const float* pr = patch + 22 * f1 + g;  // tap g + 32 i of this output frequency: row 2 f1 + kf, column kt
#pragma unroll
      for (int i = 0; i < kFeDwSlots; ++i) {
        const float xv = pr[32 * i];  // <= 22 (F1 - 1) + 31 + 448 < pw
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(d[c], xv, acc[i][c]);
      }
    }
  }
  float* o = part + (int64_t)blockIdx.x * (kFeTaps * kFeC) + 4 * cq;
#pragma unroll
  for (int i = 0; i < kFeDwSlots; ++i) {
    const int tap = g + 32 * i;
    if (tap < kFeTaps) *reinterpret_cast<f32x4*>(o + tap * kFeC) = acc[i];
  }
}

// dw[c * 451 + tap] = the sum over the partials of part[p][tap][c], in double, four strided chains joined in order
__global__ __launch_bounds__(256) void ds2_conv1_dw_join_kernel(const float* __restrict__ part, int nparts, float* __restrict__ dw) {
  __shared__ double red[4][64];
  const int l = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int o = blockIdx.x * 64 + l;  // = tap * 32 + c
  double s = 0.0;
  if (o < kFeTaps * kFeC)
    for (int p = grp; p < nparts; p += 4) s += (double)part[(int64_t)p * (kFeTaps * kFeC) + o];
  red[grp][l] = s;
  __syncthreads();
  if (grp == 0 && o < kFeTaps * kFeC) dw[(o & 31) * kFeTaps + (o >> 5)] = (float)(red[0][l] + red[1][l] + red[2][l] + red[3][l]);
}

__global__ __launch_bounds__(256) void ds2_commit_kernel(float* __restrict__ dst, const float* __restrict__ src, int n,
                                                         const int32_t* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && flag[0] == 0) dst[i] = src[i];
}

static int fe_dims(int64_t B, int32_t F, int64_t T, int* F1, int64_t* T1) {
  if (B < 1 || F < 1 || T < 1) return MA_ERR_INVALID_ARG;
  *F1 = (F - 1) / 2 + 1;
  *T1 = (T - 1) / 2 + 1;
  if (F > kFeMaxF || B > 65535 || *T1 > 0x7fffffff / 2 || B * *T1 > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  return MA_OK;
}

// workgroups of a statistics pass over n32 runs of 32 channels, and the runs each takes
static int stats_parts(int64_t n32, int64_t* per) {
  int64_t parts = (n32 + 255) / 256;
  parts = parts < 1 ? 1 : (parts > kFeMaxParts ? kFeMaxParts : parts);
  *per = (n32 + parts - 1) / parts;
  return (int)((n32 + *per - 1) / *per);
}

static int elementwise_grid(int64_t n4) {
  const int64_t g = (n4 + 255) / 256, cap = (int64_t)num_cus() * 16;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace ma

using namespace ma;

extern "C" {

int32_t ma_ds2_conv1_raw_parts(int64_t B, int64_t T) {
  if (B < 1 || T < 1 || B > 65535) return MA_ERR_INVALID_ARG;
  const int64_t T1 = (T - 1) / 2 + 1, parts = (T1 + kFeFramesPerWg - 1) / kFeFramesPerWg * B;
  return parts > 0x7fffffff ? MA_ERR_UNSUPPORTED : (int32_t)parts;
}

int ma_ds2_conv1_raw_f32(const float* x, int64_t B, int32_t F, int64_t T, const float* wt, float* y1, double* partials,
                         ma_stream_t stream) {
  if (!x || !wt || !y1 || !partials) return MA_ERR_INVALID_ARG;
  int F1 = 0;
  int64_t T1 = 0;
  const int rc = fe_dims(B, F, T, &F1, &T1);
  if (rc != MA_OK) return rc;
  const int lds = kFeTaps * kFeC * 4 + (F + 40) * kFeKt * 4;
  MA_LAUNCH(ds2_conv1_raw_kernel, dim3((unsigned)((T1 + kFeFramesPerWg - 1) / kFeFramesPerWg), (unsigned)B), dim3(256), lds,
            (hipStream_t)stream, x, F, (int)T, (int)B, F1, (int)T1, wt, y1, partials);
  return MA_OK;
}

int32_t ma_ds2_stats_parts(int64_t n) {
  if (n < 32 || n % 32) return MA_ERR_INVALID_ARG;
  int64_t per = 0;
  return stats_parts(n / 32, &per);
}

int ma_ds2_bn_stats_f32(const float* y, int64_t n, double* partials, ma_stream_t stream) {
  if (!y || !partials || n < 32 || n % 32 || (reinterpret_cast<uintptr_t>(y) & 15)) return MA_ERR_INVALID_ARG;
  int64_t per = 0;
  const int parts = stats_parts(n / 32, &per);
  MA_LAUNCH(ds2_stats_kernel, dim3((unsigned)parts), dim3(256), 0, (hipStream_t)stream, y, n / 32, per, partials);
  return MA_OK;
}

int ma_ds2_bn_finalize_f32(const double* partials, int32_t nparts, int64_t count, float eps, float momentum, const float* mean_in,
                           const float* var_in, float* mean_out, float* var_out, float* stats, ma_stream_t stream) {
  if (!partials || !stats || nparts < 1 || count < 1) return MA_ERR_INVALID_ARG;
  if ((mean_out != nullptr) != (var_out != nullptr) || (mean_out && (!mean_in || !var_in))) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(ds2_bn_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nparts, (double)count, eps, momentum, mean_in,
            var_in, mean_out, var_out, stats);
  return MA_OK;
}

static int bn_image_check(const void* y, int64_t rows, int32_t cols, const void* out, int64_t ldo, int64_t align) {
  if (!y || !out || rows < 1 || cols < 32 || cols % 32) return MA_ERR_INVALID_ARG;
  if (ldo < cols || (ldo & 3) || rows * (cols / 4) > ((int64_t)1 << 40)) return MA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(y) & 15) || (reinterpret_cast<uintptr_t>(out) & (align - 1))) return MA_ERR_INVALID_ARG;
  return MA_OK;
}

int ma_ds2_bn_tanh_fwd_bf16(const float* y, int64_t rows, int32_t cols, const float* stats, const float* gamma, const float* beta,
                            void* out, int64_t ldo, ma_stream_t stream) {
  if (!stats || !gamma || !beta) return MA_ERR_INVALID_ARG;
  const int rc = bn_image_check(y, rows, cols, out, ldo, 8);
  if (rc != MA_OK) return rc;
  MA_LAUNCH(ds2_bn_tanh_fwd_kernel, dim3((unsigned)elementwise_grid(rows * (cols / 4))), dim3(256), 0, (hipStream_t)stream, y, rows,
            (int)cols, stats, gamma, beta, reinterpret_cast<uint16_t*>(out), ldo);
  return MA_OK;
}

int64_t ma_ds2_bn_tanh_bwd_workspace_bytes(int64_t rows, int32_t cols) {
  if (rows < 1 || cols < 32 || cols % 32) return MA_ERR_INVALID_ARG;
  int64_t per = 0;
  return (int64_t)stats_parts(rows * (cols / 32), &per) * 64 * 8;
}

int ma_ds2_bn_tanh_bwd_f32(const float* y, const float* dout, int64_t ldd, int64_t rows, int32_t cols, const float* stats,
                           const float* gamma, const float* beta, void* out, int64_t ldo, int32_t out_bf16, float* bsum, float* d_gamma,
                           float* d_beta, void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  if (!stats || !gamma || !beta || !dout || !bsum || !workspace) return MA_ERR_INVALID_ARG;
  const int rc = bn_image_check(y, rows, cols, out, ldo, out_bf16 ? 8 : 16);
  if (rc != MA_OK) return rc;
  if (ldd < cols || (ldd & 3) || (reinterpret_cast<uintptr_t>(dout) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return MA_ERR_INVALID_ARG;
  const int64_t n32 = rows * (cols / 32);
  int64_t per = 0;
  const int parts = stats_parts(n32, &per);
  if (workspace_bytes < (int64_t)parts * 64 * 8) return MA_ERR_WORKSPACE;
  double* part = reinterpret_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  MA_LAUNCH(ds2_bn_tanh_bwd1_kernel, dim3((unsigned)parts), dim3(256), 0, s, y, dout, ldd, n32, (int)(cols / 32), per, stats, gamma, beta,
            part);
  MA_LAUNCH(ds2_bn_bwd_join_kernel, dim3(1), dim3(256), 0, s, (const double*)part, parts, (double)rows * (double)(cols / 32), bsum, d_gamma,
            d_beta);
  const unsigned grid = (unsigned)elementwise_grid(rows * (cols / 4));
  if (out_bf16)
    MA_LAUNCH(ds2_bn_tanh_bwd2_kernel<true>, dim3(grid), dim3(256), 0, s, y, dout, ldd, rows, (int)cols, stats, gamma, beta,
              (const float*)bsum, out, ldo);
  else
    MA_LAUNCH(ds2_bn_tanh_bwd2_kernel<false>, dim3(grid), dim3(256), 0, s, y, dout, ldd, rows, (int)cols, stats, gamma, beta,
              (const float*)bsum, out, ldo);
  return MA_OK;
}

int32_t ma_ds2_conv1_dw_parts(int64_t B, int64_t T, int32_t frames_per_wg) {
  if (B < 1 || T < 1 || frames_per_wg < 0) return MA_ERR_INVALID_ARG;
  const int64_t frames = B * ((T - 1) / 2 + 1);
  const int64_t fpw = frames_per_wg > 0 ? frames_per_wg : (frames + kFeMaxParts - 1) / kFeMaxParts;
  const int64_t parts = (frames + fpw - 1) / fpw;
  return parts > 65535 * 16 ? MA_ERR_UNSUPPORTED : (int32_t)parts;
}

int ma_ds2_conv1_dw_f32(const float* x, int64_t B, int32_t F, int64_t T, const float* dz1, int32_t frames_per_wg, float* dw,
                        void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  if (!x || !dz1 || !dw || !workspace || frames_per_wg < 0) return MA_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(dz1) | reinterpret_cast<uintptr_t>(workspace)) & 15) return MA_ERR_INVALID_ARG;
  int F1 = 0;
  int64_t T1 = 0;
  const int rc = fe_dims(B, F, T, &F1, &T1);
  if (rc != MA_OK) return rc;
  const int parts = ma_ds2_conv1_dw_parts(B, T, frames_per_wg);
  if (parts < 1) return parts;
  const int64_t frames = B * T1;
  const int fpw = (int)(frames_per_wg > 0 ? frames_per_wg : (frames + kFeMaxParts - 1) / kFeMaxParts);
  if (workspace_bytes < (int64_t)parts * kFeTaps * kFeC * 4) return MA_ERR_WORKSPACE;
  float* part = reinterpret_cast<float*>(workspace);
  const int lds = (fe_dw_patch_words(F) + F1 * kFeC) * 4;
  MA_LAUNCH(ds2_conv1_dw_kernel, dim3((unsigned)parts), dim3(256), lds, (hipStream_t)stream, x, F, (int)T, (int)B, F1, (int)T1, dz1, fpw,
            part);
  MA_LAUNCH(ds2_conv1_dw_join_kernel, dim3((kFeTaps * kFeC + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const float*)part, parts, dw);
  return MA_OK;
}

int ma_ds2_commit_f32(float* dst, const float* src, int32_t n, const int32_t* overflow, ma_stream_t stream) {
  if (!dst || !src || !overflow || n < 1) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(ds2_commit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, src, (int)n, overflow);
  return MA_OK;
}

}  // extern "C"
