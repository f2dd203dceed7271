// WaveGrad training (examples/wavegrad/train.py around mindaudio/models/wavegrad/wavegrad_v190.py): everything of the backward pass
// and of the optimizer step that is no MFMA product.  Contract: include/mindaudio_amd.h.  The products are ma_conv1d_taps_bf16 /
// ma_gemm_bf16 / ma_gemm_tn_bf16_f32 (ma_gemm_x32 in float32 mode) calls of the trainer, on operand images that
// ma_wavegrad_pack_bf16 / ma_wavegrad_pack_f32 write.
//
// wt_l1_last_bwd_kernel: one workgroup per 64 samples of one utterance (the grid of wg_last_conv_kernel).  g = sign(pred - noise) *
//   gscale for its rows and the taps - 1 rows around them sits in LDS; dx is an fma chain over the taps per (row, 4 channels); the
//   weight-gradient partial of the workgroup is formed by (channel group, row subset) threads and joined through LDS in subset order.
// wt_pack_bwd_kernel: one thread per (input row, 4 channels), a loop over the f repeated output rows.
// wt_init_bwd_kernel: one workgroup per 256 samples of one utterance, the same (channel group, row subset) scheme.
// wt_sumsq_kernel / wt_clip_adam_kernel: float64 partials of sum g^2; every workgroup of the update joins them in the same order.
// wt_weights_kernel: the bf16 operand copies of all convolutions from the float32 masters in one launch.
// No atomics; every sum has a fixed order.  All bandwidth-bound.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kWtThreads = 256;
constexpr int kWtMaxTaps = 7;
constexpr int kWtLastRows = 64;
constexpr int kWtInitRows = 256;
constexpr int kWtAcc = kWtMaxTaps + 1;  // accumulator rows of a thread: the taps and (init) the bias
constexpr int kWtMaxParts = 1024;       // partials of sum g^2
constexpr float kWtInvSqrt2 = 0.70710678118654752440f;

// Joins the per-thread accumulators acc[a][0..3] (a < na; thread = (channel group cg, row subset rs)) of a workgroup: through LDS,
// subsets added in order, -> out[a * C + c].  red holds kWtAcc * 4 * kWtThreads floats.
__device__ __forceinline__ void wt_join_subsets(float (&acc)[kWtAcc][4], int na, int C, int cg, int rs, int nrs, bool active, float* red,
                                                float* __restrict__ out) {
  if (active) {
#pragma unroll
    for (int a = 0; a < kWtAcc; ++a)
      if (a < na) *reinterpret_cast<f32x4*>(red + ((int64_t)rs * na + a) * C + cg * 4) = (f32x4){acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
  }
  __syncthreads();
  for (int i = threadIdx.x; i < na * C; i += kWtThreads) {
    float s = 0.0f;
    for (int k = 0; k < nrs; ++k) s += red[(int64_t)k * na * C + i];
    out[i] = s;
  }
}

__global__ __launch_bounds__(kWtThreads) void wt_l1_last_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ noise,
                                                                    const float* __restrict__ x, const float* __restrict__ w, int64_t T,
                                                                    int C, int taps, float gscale, float* __restrict__ g_out,
                                                                    float* __restrict__ dx, float* __restrict__ wpart, int64_t pstride,
                                                                    double* __restrict__ loss_part) {
  __shared__ float g_s[kWtLastRows + kWtMaxTaps - 1];
  __shared__ float red[kWtAcc * 4 * kWtThreads];
  const int64_t t0 = (int64_t)blockIdx.x * kWtLastRows, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = taps >> 1;
  const int64_t wg = b * gridDim.x + blockIdx.x;
  if (tid < kWtLastRows + taps - 1) {  // g_s[i] is the gradient at t0 + i - half; zero outside the utterance
    const int64_t tt = t0 + tid - half;
    float gv = 0.0f;
    if (tt >= 0 && tt < T) {
      const float d = pred[b * T + tt] - noise[b * T + tt];
      gv = d > 0.0f ? gscale : (d < 0.0f ? -gscale : 0.0f);  // sign(0) = 0
    }
    g_s[tid] = gv;
  }
  if (wave == 0) {  // the workgroup's own 64 rows: the loss partial, the bias-gradient partial and g itself
    const int64_t t = t0 + lane;
    double a = 0.0;
    float gv = 0.0f;
    if (t < T) {
      const float d = pred[b * T + t] - noise[b * T + t];
      a = (double)fabsf(d);
      gv = d > 0.0f ? gscale : (d < 0.0f ? -gscale : 0.0f);
      g_out[b * T + t] = gv;
    }
    a = wave_sum(a);
    gv = wave_sum(gv);
    if (lane == 0) {
      loss_part[wg] = a;
      wpart[wg * pstride + (int64_t)taps * C] = gv;
    }
  }
  __syncthreads();
  // dx[b, t, c] = sum_j g[t - (j - half)] w[j, c]: g_s index r + taps - 1 - j
  for (int r = wave; r < kWtLastRows; r += kWtThreads / 64) {
    const int64_t t = t0 + r;
    if (t >= T) break;
    for (int c = lane * 4; c < C; c += 256) {
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < kWtMaxTaps; ++j)
        if (j < taps) {
          const float gv = g_s[r + taps - 1 - j];
          const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (int64_t)j * C + c);
          acc.x = fmaf(gv, wv.x, acc.x);
          acc.y = fmaf(gv, wv.y, acc.y);
          acc.z = fmaf(gv, wv.z, acc.z);
          acc.w = fmaf(gv, wv.w, acc.w);
        }
      *reinterpret_cast<f32x4*>(dx + (b * T + t) * C + c) = acc;
    }
  }
  // dw[j, c] partial = sum over the rows of g[t] x[b, t + j - half, c]
  const int ncg = C >> 2, nrs = kWtThreads / ncg;
  const int cg = tid % ncg, rs = tid / ncg;
  const bool active = rs < nrs;
  float acc[kWtAcc][4];
#pragma unroll
  for (int a = 0; a < kWtAcc; ++a) acc[a][0] = acc[a][1] = acc[a][2] = acc[a][3] = 0.0f;
  if (active)
    for (int r = rs; r < kWtLastRows && t0 + r < T; r += nrs) {
      const float gv = g_s[r + half];
#pragma unroll
      for (int j = 0; j < kWtMaxTaps; ++j)
        if (j < taps) {
          const int64_t tt = t0 + r + j - half;
          if (tt >= 0 && tt < T) {  // rows outside the utterance are zero
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (b * T + tt) * C + cg * 4);
            acc[j][0] = fmaf(gv, xv.x, acc[j][0]);
            acc[j][1] = fmaf(gv, xv.y, acc[j][1]);
            acc[j][2] = fmaf(gv, xv.z, acc[j][2]);
            acc[j][3] = fmaf(gv, xv.w, acc[j][3]);
          }
        }
    }
  wt_join_subsets(acc, taps, C, cg, rs, nrs, active, red, wpart + wg * pstride);
}

// loss[0] = sum of the partials / count, in one fixed order (thread-strided sums, the butterfly of a wave, the four waves in order)
__global__ __launch_bounds__(kWtThreads) void wt_l1_join_kernel(const double* __restrict__ part, int64_t n, double count,
                                                                double* __restrict__ loss) {
  __shared__ double s4[kWtThreads / 64];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kWtThreads) s += part[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (((s4[0] + s4[1]) + s4[2]) + s4[3]) / count;
}

__global__ __launch_bounds__(kWtThreads) void wt_pack_bwd_kernel(const float* __restrict__ dop, int64_t ld_dop, const float* __restrict__ x,
                                                                 int64_t T_in, int f, int C, const float* __restrict__ film,
                                                                 int64_t ld_film, float slope, float mul, const float* __restrict__ dres,
                                                                 float res_mul, float* __restrict__ dx, int acc_dx,
                                                                 float* __restrict__ dfilm, int64_t ld_dfilm, int acc_film, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kWtThreads + threadIdx.x;
  if (idx >= total) return;
  const int c4n = C >> 2;
  const int c = (int)(idx % c4n) * 4;
  const int64_t irow = idx / c4n;  // b * T_in + t_in; its output rows are irow * f .. irow * f + f - 1
  const f32x4 xv = *reinterpret_cast<const f32x4*>(x + irow * C + c);
  const float v[4] = {xv.x, xv.y, xv.z, xv.w};
  float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < f; ++k) {
    const int64_t orow = irow * f + k;
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (dop) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(dop + orow * ld_dop + c);
      const float dv[4] = {d.x, d.y, d.z, d.w};
      float sc[4] = {1.0f, 1.0f, 1.0f, 1.0f}, pre[4] = {v[0], v[1], v[2], v[3]};
      if (film) {
        const float* fp = film + orow * ld_film + c;
        const f32x4 h = *reinterpret_cast<const f32x4*>(fp), s = *reinterpret_cast<const f32x4*>(fp + C);
        const float sh[4] = {h.x, h.y, h.z, h.w};
        sc[0] = s.x, sc[1] = s.y, sc[2] = s.z, sc[3] = s.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[i] = fmaf(sc[i], v[i], sh[i]) * kWtInvSqrt2;  // the forward's value, bit for bit
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) g[i] = (dv[i] * mul) * (pre[i] >= 0.0f ? 1.0f : slope);
      if (film) {
        float dsh[4], dsc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dsh[i] = g[i] * kWtInvSqrt2;
          dsc[i] = (g[i] * v[i]) * kWtInvSqrt2;
          g[i] = (g[i] * sc[i]) * kWtInvSqrt2;
        }
        if (dfilm) {
          float* dp = dfilm + orow * ld_dfilm + c;
          f32x4 a = {dsh[0], dsh[1], dsh[2], dsh[3]}, s = {dsc[0], dsc[1], dsc[2], dsc[3]};
          if (acc_film) {
            const f32x4 oa = *reinterpret_cast<const f32x4*>(dp), os = *reinterpret_cast<const f32x4*>(dp + C);
            a = (f32x4){oa.x + a.x, oa.y + a.y, oa.z + a.z, oa.w + a.w};
            s = (f32x4){os.x + s.x, os.y + s.y, os.z + s.z, os.w + s.w};
          }
          *reinterpret_cast<f32x4*>(dp) = a;
          *reinterpret_cast<f32x4*>(dp + C) = s;
        }
      }
    }
    if (dres) {
      const f32x4 d = *reinterpret_cast<const f32x4*>(dres + orow * C + c);
      g[0] = fmaf(d.x, res_mul, g[0]);
      g[1] = fmaf(d.y, res_mul, g[1]);
      g[2] = fmaf(d.z, res_mul, g[2]);
      g[3] = fmaf(d.w, res_mul, g[3]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += g[i];
  }
  if (dx) {
    float* o = dx + irow * C + c;
    f32x4 r = {sum[0], sum[1], sum[2], sum[3]};
    if (acc_dx) {
      const f32x4 old = *reinterpret_cast<const f32x4*>(o);
      r = (f32x4){old.x + r.x, old.y + r.y, old.z + r.z, old.w + r.w};
    }
    *reinterpret_cast<f32x4*>(o) = r;
  }
}

// partial of workgroup (tile, b): [taps][C0] sums of dout[b, t, c] audio[b, t + j - half], then [C0] sums of dout[b, t, c]
__global__ __launch_bounds__(kWtThreads) void wt_init_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ audio, int64_t T,
                                                                 int taps, int C0, float* __restrict__ part) {
  __shared__ float red[kWtAcc * 4 * kWtThreads];
  const int64_t t0 = (int64_t)blockIdx.x * kWtInitRows, b = blockIdx.y;
  const int tid = threadIdx.x, half = taps >> 1;
  const int ncg = C0 >> 2, nrs = kWtThreads / ncg;
  const int cg = tid % ncg, rs = tid / ncg;
  const bool active = rs < nrs;
  float acc[kWtAcc][4];
#pragma unroll
  for (int a = 0; a < kWtAcc; ++a) acc[a][0] = acc[a][1] = acc[a][2] = acc[a][3] = 0.0f;
  if (active)
    for (int r = rs; r < kWtInitRows && t0 + r < T; r += nrs) {
      const int64_t t = t0 + r;
      const f32x4 d = *reinterpret_cast<const f32x4*>(dout + (b * T + t) * C0 + cg * 4);
#pragma unroll
      for (int j = 0; j < kWtMaxTaps; ++j)
        if (j < taps) {
          const int64_t tt = t + j - half;
          const float a = (tt >= 0 && tt < T) ? audio[b * T + tt] : 0.0f;
          acc[j][0] = fmaf(d.x, a, acc[j][0]);
          acc[j][1] = fmaf(d.y, a, acc[j][1]);
          acc[j][2] = fmaf(d.z, a, acc[j][2]);
          acc[j][3] = fmaf(d.w, a, acc[j][3]);
        }
      // the bias row sits behind the taps
#pragma unroll
      for (int j = 0; j < kWtAcc; ++j)
        if (j == taps) {
          acc[j][0] += d.x;
          acc[j][1] += d.y;
          acc[j][2] += d.z;
          acc[j][3] += d.w;
        }
    }
  wt_join_subsets(acc, taps + 1, C0, cg, rs, nrs, active, red, part + (b * gridDim.x + blockIdx.x) * (int64_t)(taps + 1) * C0);
}

__global__ __launch_bounds__(kWtThreads) void wt_sumsq_kernel(const float* __restrict__ g, int64_t n4, double* __restrict__ part) {
  __shared__ double s4[kWtThreads / 64];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kWtThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kWtThreads) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + i * 4);
    s += (double)v.x * v.x;
    s += (double)v.y * v.y;
    s += (double)v.z * v.z;
    s += (double)v.w * v.w;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// ops.clip_by_global_norm behind the unscaling, then nn.Adam as ma_adam_f32 states it (adam_one of train_kernels.hip, restated here
// because the factor sits between the unscaling and the moments).
__global__ __launch_bounds__(kWtThreads) void wt_clip_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                  float* __restrict__ v, int64_t n4, const double* __restrict__ part,
                                                                  int n_parts, float loss_scale, float clip, float lr_t, float b1, float b2,
                                                                  float eps, int32_t* __restrict__ overflow, float* __restrict__ norm_out) {
  __shared__ double s4[kWtThreads / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_parts; i += kWtThreads) s += part[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = s;
  __syncthreads();
  const double norm = sqrt(((s4[0] + s4[1]) + s4[2]) + s4[3]) / (double)loss_scale;  // the same bits in every workgroup
  const bool bad = !(norm <= 1.7976931348623157e308);                                // inf or nan
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    overflow[0] = bad ? 1 : 0;
    norm_out[0] = (float)norm;
  }
  if (bad) return;
  const float factor = (float)((double)clip / fmax(norm, (double)clip));
  const float inv_scale = 1.0f / loss_scale;
  for (int64_t i = (int64_t)blockIdx.x * kWtThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kWtThreads) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 pv = *reinterpret_cast<const f32x4*>(p + i * 4), mv = *reinterpret_cast<const f32x4*>(m + i * 4),
          vv = *reinterpret_cast<const f32x4*>(v + i * 4);
    const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
    float pe[4] = {pv.x, pv.y, pv.z, pv.w}, me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gi = (ge[k] * inv_scale) * factor;
      const float mi = b1 * me[k] + (1.0f - b1) * gi;
      const float vi = b2 * ve[k] + (1.0f - b2) * gi * gi;
      me[k] = mi;
      ve[k] = vi;
      pe[k] -= lr_t * mi / (sqrtf(vi) + eps);
    }
    *reinterpret_cast<f32x4*>(m + i * 4) = (f32x4){me[0], me[1], me[2], me[3]};
    *reinterpret_cast<f32x4*>(v + i * 4) = (f32x4){ve[0], ve[1], ve[2], ve[3]};
    *reinterpret_cast<f32x4*>(p + i * 4) = (f32x4){pe[0], pe[1], pe[2], pe[3]};
  }
}

__global__ __launch_bounds__(kWtThreads) void wt_weights_kernel(const ma_wavegrad_weight_item_t* __restrict__ items,
                                                                const int32_t* __restrict__ block_item) {
  const ma_wavegrad_weight_item_t it = items[block_item[blockIdx.x]];
  const int64_t idx = (int64_t)((int)blockIdx.x - it.first_block) * kWtThreads + threadIdx.x;
  const int64_t total = (int64_t)it.Npad * it.taps * it.Cpad;
  if (idx >= total) return;
  const int c = (int)(idx % it.Cpad);
  const int j = (int)((idx / it.Cpad) % it.taps);
  const int n = (int)(idx / ((int64_t)it.Cpad * it.taps));
  const float val = (n < it.N && c < it.C) ? it.src[((int64_t)n * it.taps + j) * it.C + c] : 0.0f;
  const uint16_t h = f2bf(val);
  if (it.fwd && n < it.rows_fwd) reinterpret_cast<uint16_t*>(it.fwd)[((int64_t)n * it.taps + j) * it.Cpad + c] = h;
  if (it.rev) {
    uint16_t* rev = reinterpret_cast<uint16_t*>(it.rev);
    if (it.mode == 1)
      rev[((int64_t)j * it.Cpad + c) * it.Npad + n] = h;  // (taps * Cpad, Npad): the transposed matrix of a kernel = stride convolution
    else if (c < it.C)
      rev[((int64_t)c * it.taps + (it.taps - 1 - j)) * it.Npad + n] = h;  // (C, taps, Npad), taps reversed
  }
}

// float32 image of the operand producer (the validation mode): wg_pack_kernel's arithmetic without the final rounding
__global__ __launch_bounds__(kWtThreads) void wt_pack_f32_kernel(const float* __restrict__ x, int64_t T_in, int64_t T_out, int f, int C, int halo,
                                                                 const float* __restrict__ film, int64_t ld_film,
                                                                 const float* __restrict__ enc, int64_t ld_enc, float slope, float mul,
                                                                 float* __restrict__ out, float* __restrict__ res, float res_mul,
                                                                 int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kWtThreads + threadIdx.x;
  if (idx >= total) return;
  const int c4n = C >> 2;
  const int c = (int)(idx % c4n) * 4;
  const int64_t row = idx / c4n;  // b * (T_out + 2 halo) + r
  const int64_t rows_u = T_out + 2 * (int64_t)halo;
  const int64_t b = row / rows_u, t = row - b * rows_u - halo;
  f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
  if (t >= 0 && t < T_out) {
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(x + (b * T_in + t / f) * C + c);
    float v[4] = {x0.x, x0.y, x0.z, x0.w};
    const int64_t orow = b * T_out + t;
    if (res) *reinterpret_cast<f32x4*>(res + orow * C + c) = (f32x4){v[0] * res_mul, v[1] * res_mul, v[2] * res_mul, v[3] * res_mul};
    if (film) {
      const float* fp = film + orow * ld_film + c;
      const f32x4 h = *reinterpret_cast<const f32x4*>(fp), s = *reinterpret_cast<const f32x4*>(fp + C);
      const float sh[4] = {h.x, h.y, h.z, h.w}, sc[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaf(sc[i], v[i], sh[i]) * kWtInvSqrt2;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] >= 0.0f ? v[i] : slope * v[i];
    if (enc) {
      const f32x4 e = *reinterpret_cast<const f32x4*>(enc + b * ld_enc + c);
      v[0] += e.x, v[1] += e.y, v[2] += e.z, v[3] += e.w;
    }
    o = (f32x4){v[0] * mul, v[1] * mul, v[2] * mul, v[3] * mul};
  }
  if (out) *reinterpret_cast<f32x4*>(out + row * C + c) = o;
}

static inline bool wt_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace ma

using namespace ma;

extern "C" {

int32_t ma_wavegrad_last_bwd_parts(int64_t B, int64_t T) {
  if (B < 1 || T < 1) return MA_ERR_INVALID_ARG;
  const int64_t n = B * ((T + kWtLastRows - 1) / kWtLastRows);
  return n > 0x7fffffff ? MA_ERR_UNSUPPORTED : (int32_t)n;
}

int32_t ma_wavegrad_init_bwd_parts(int64_t B, int64_t T) {
  if (B < 1 || T < 1) return MA_ERR_INVALID_ARG;
  const int64_t n = B * ((T + kWtInitRows - 1) / kWtInitRows);
  return n > 0x7fffffff ? MA_ERR_UNSUPPORTED : (int32_t)n;
}

int ma_wavegrad_l1_last_bwd_f32(const float* pred, const float* noise, const float* x, int64_t B, int64_t T, int32_t C, const float* w,
                                int32_t taps, float loss_scale, float* g, float* dx, float* wpart, int64_t pstride, double* loss_part,
                                double* loss, ma_stream_t stream) {
  if (!pred || !noise || !x || !w || !g || !dx || !wpart || !loss_part || !loss || B < 1 || T < 1 || C < 1 || taps < 1 || !(taps & 1) ||
      pstride < (int64_t)taps * C + 1)
    return MA_ERR_INVALID_ARG;
  if (wt_misaligned(x) || wt_misaligned(w) || wt_misaligned(dx) || wt_misaligned(wpart)) return MA_ERR_INVALID_ARG;
  if (taps > kWtMaxTaps || (C & 3) || C > 4 * kWtThreads || B > 65535 || (pstride & 3)) return MA_ERR_UNSUPPORTED;
  const int64_t blocks = (T + kWtLastRows - 1) / kWtLastRows;
  if (blocks * B > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  const float gscale = (float)((double)loss_scale / ((double)B * (double)T));
  MA_LAUNCH(wt_l1_last_bwd_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(kWtThreads), 0, (hipStream_t)stream, pred, noise, x, w, T, C,
            taps, gscale, g, dx, wpart, pstride, loss_part);
  MA_LAUNCH(wt_l1_join_kernel, dim3(1), dim3(kWtThreads), 0, (hipStream_t)stream, loss_part, blocks * B, (double)B * (double)T, loss);
  return MA_OK;
}

int ma_wavegrad_pack_bwd_f32(const float* dop, int64_t ld_dop, const float* x, int64_t B, int64_t T_in, int32_t f, int32_t C,
                             const float* film, int64_t ld_film, float slope, float mul, const float* dres, float res_mul, float* dx,
                             int32_t acc_dx, float* dfilm, int64_t ld_dfilm, int32_t acc_film, ma_stream_t stream) {
  if (!x || (!dop && !dres) || (!dx && !dfilm) || B < 1 || T_in < 1 || f < 1 || C < 1) return MA_ERR_INVALID_ARG;
  if ((dop && ld_dop < C) || (film && ld_film < 2 * (int64_t)C) || (dfilm && (!film || !dop || ld_dfilm < 2 * (int64_t)C)))
    return MA_ERR_INVALID_ARG;
  if (wt_misaligned(dop) || wt_misaligned(x) || wt_misaligned(film) || wt_misaligned(dres) || wt_misaligned(dx) || wt_misaligned(dfilm))
    return MA_ERR_INVALID_ARG;
  if ((C & 3) || (dop && (ld_dop & 3)) || (film && (ld_film & 3)) || (dfilm && (ld_dfilm & 3))) return MA_ERR_UNSUPPORTED;
  const int64_t total = B * T_in * (C >> 2), blocks = (total + kWtThreads - 1) / kWtThreads;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(wt_pack_bwd_kernel, dim3((unsigned)blocks), dim3(kWtThreads), 0, (hipStream_t)stream, dop, ld_dop, x, T_in, f, C, film, ld_film,
            slope, mul, dres, res_mul, dx, acc_dx, dfilm, ld_dfilm, acc_film, total);
  return MA_OK;
}

int ma_wavegrad_init_conv_bwd_f32(const float* dout, const float* audio, int64_t B, int64_t T, int32_t taps, int32_t C0, float* part,
                                  ma_stream_t stream) {
  if (!dout || !audio || !part || B < 1 || T < 1 || C0 < 1 || taps < 1 || !(taps & 1)) return MA_ERR_INVALID_ARG;
  if (wt_misaligned(dout) || wt_misaligned(part)) return MA_ERR_INVALID_ARG;
  if (taps > kWtMaxTaps || (C0 & 3) || C0 > 4 * kWtThreads || B > 65535) return MA_ERR_UNSUPPORTED;
  const int64_t blocks = (T + kWtInitRows - 1) / kWtInitRows;
  if (blocks * B > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(wt_init_bwd_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(kWtThreads), 0, (hipStream_t)stream, dout, audio, T, taps, C0, part);
  return MA_OK;
}

int32_t ma_wavegrad_sumsq_parts(int64_t n) {
  if (n < 1) return MA_ERR_INVALID_ARG;
  const int64_t blocks = (n / 4 + kWtThreads * 16 - 1) / (kWtThreads * 16);
  return (int32_t)(blocks < 1 ? 1 : (blocks > kWtMaxParts ? kWtMaxParts : blocks));
}

int ma_wavegrad_sumsq_f64(const float* g, int64_t n, double* part, ma_stream_t stream) {
  if (!g || !part || n < 1) return MA_ERR_INVALID_ARG;
  if (wt_misaligned(g)) return MA_ERR_INVALID_ARG;
  if (n & 3) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(wt_sumsq_kernel, dim3((unsigned)ma_wavegrad_sumsq_parts(n)), dim3(kWtThreads), 0, (hipStream_t)stream, g, n / 4, part);
  return MA_OK;
}

int ma_wavegrad_clip_adam_f32(float* param, const float* grad, float* m, float* v, int64_t n, const double* part, int32_t n_parts,
                              float loss_scale, float clip, float lr_t, float beta1, float beta2, float eps, int32_t* overflow,
                              float* norm, ma_stream_t stream) {
  if (!param || !grad || !m || !v || !part || !overflow || !norm || n < 1 || n_parts < 1 || !(loss_scale > 0.0f) || !(clip > 0.0f))
    return MA_ERR_INVALID_ARG;
  if (wt_misaligned(param) || wt_misaligned(grad) || wt_misaligned(m) || wt_misaligned(v)) return MA_ERR_INVALID_ARG;
  if ((n & 3) || n_parts > kWtMaxParts) return MA_ERR_UNSUPPORTED;
  int64_t blocks = (n / 4 + kWtThreads - 1) / kWtThreads;
  if (blocks > 4096) blocks = 4096;
  MA_LAUNCH(wt_clip_adam_kernel, dim3((unsigned)blocks), dim3(kWtThreads), 0, (hipStream_t)stream, param, grad, m, v, n / 4, part, n_parts,
            loss_scale, clip, lr_t, beta1, beta2, eps, overflow, norm);
  return MA_OK;
}

int ma_wavegrad_weights_bf16(const ma_wavegrad_weight_item_t* items, const int32_t* block_item, int32_t n_blocks, ma_stream_t stream) {
  if (!items || !block_item || n_blocks < 1) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(wt_weights_kernel, dim3((unsigned)n_blocks), dim3(kWtThreads), 0, (hipStream_t)stream, items, block_item);
  return MA_OK;
}

int ma_wavegrad_pack_f32(const float* x, int64_t B, int64_t T_in, int32_t f, int32_t C, int32_t halo, const float* film, int64_t ld_film,
                         const float* enc, int64_t ld_enc, float slope, float mul, float* out, float* res, float res_mul,
                         ma_stream_t stream) {
  if (!x || (!out && !res) || B < 1 || T_in < 1 || f < 1 || C < 1 || halo < 0) return MA_ERR_INVALID_ARG;
  if (film && ld_film < 2 * (int64_t)C) return MA_ERR_INVALID_ARG;
  if (enc && ld_enc != 0 && ld_enc < C) return MA_ERR_INVALID_ARG;
  if (wt_misaligned(x) || wt_misaligned(film) || wt_misaligned(enc) || wt_misaligned(out) || wt_misaligned(res)) return MA_ERR_INVALID_ARG;
  if ((C & 3) || (film && (ld_film & 3)) || (enc && (ld_enc & 3))) return MA_ERR_UNSUPPORTED;
  const int64_t T_out = T_in * f;
  const int64_t total = B * (T_out + 2 * (int64_t)halo) * (C >> 2), blocks = (total + kWtThreads - 1) / kWtThreads;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(wt_pack_f32_kernel, dim3((unsigned)blocks), dim3(kWtThreads), 0, (hipStream_t)stream, x, T_in, T_out, f, C, halo, film, ld_film, enc,
            ld_enc, slope, mul, out, res, res_mul, total);
  return MA_OK;
}

}  // extern "C"
