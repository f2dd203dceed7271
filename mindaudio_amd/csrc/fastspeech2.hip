// FastSpeech2 inference (mindaudio/models/fastspeech2/{fastspeech2_v190,variance_adapter}.py, mindaudio/models/transformer/): everything
// between its MFMA products, the key-padding-masked attention, and the host loop that walks one FFT-block stack.  Contract:
// include/mindaudio_amd.h.  The dense layers and convolutions are ma_gemm_bf16 / ma_conv1d_taps_bf16 calls (gemm_bf16.hip).
//
// fs2_mha_kernel<DK>: one wave per 16 query rows of one (utterance, head), two waves a workgroup.  Keys are walked in tiles of 32 with an
//   online softmax.  Both products run on mfma_f32_16x16x32_bf16 in the orientation that keeps the query on the lane (lane & 15):
//   S^T = K . Q^T (A = 16 key rows straight from global memory, 16 bytes a lane; B = the wave's Q fragments, loaded once), and
//   O^T = V^T . P^T (A = V^T from the workgroup's LDS image vt[d][key], B = the probabilities, which the first product left in exactly
//   the lanes the second wants: element j of lane group g is key 4 g + j (j < 4) or 16 + 4 g + (j - 4), and the V^T fragment is read in
//   that same key order).  Running max, sum and the accumulator are float32 and need no cross-lane move for the rescale.  A masked key
//   has probability exactly 0 (a select, not exp(-big)), its V row is staged as zeros, and its score is never looked at.
// fs2_gn_stats_kernel / fs2_gn_apply_kernel: GroupNorm over (T x C / G) per (utterance, group).  Each workgroup takes 64 rows and writes
//   the float64 mean and centred second moment of each group (two passes over its rows, fixed summation order); the apply launch joins
//   the partials in part order (Chan's update) and writes the float32 stream and the bf16 operand image in one pass.
// fs2_rowln_kernel: LayerNorm of one row per wave into the float32 stream and / or the bf16 operand image (zero halo rows).
// fs2_head_kernel: the tail of a VariancePredictor and its consumer, one row per wave.
// fs2_embed_kernel, fs2_duration_kernel, fs2_length_regulate_kernel: the small integer ends of the network.
// No atomics, no cross-workgroup waiting: the same bits from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kFsThreads = 256;
constexpr int kFsMhaWaves = 2;       // 16 query rows each
constexpr int kFsKeyTile = 32;
constexpr int kFsVtLd = 40;          // bf16 per row of the V^T image: 32 keys + 8 (80-byte rows keep the 8-byte reads aligned)
constexpr int kFsStatRows = 64;      // rows of one GroupNorm partial
constexpr int kFsMaxSrc = 4096;      // phonemes per utterance the length regulator holds in LDS
constexpr int kFsMaxDur = 1 << 18;   // a duration above this is clamped (kFsMaxSrc of them still fit an int32 sum)

template <int DK>
__global__ __launch_bounds__(kFsMhaWaves * 64) void fs2_mha_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                                   const uint16_t* __restrict__ v, int64_t ldq, int64_t ldk, int64_t ldv,
                                                                   const int32_t* __restrict__ lens, int T, int64_t rows_in, float scale,
                                                                   uint16_t* __restrict__ ctx, int64_t ldc, int64_t rows_out) {
  constexpr int KS = DK / 32;  // k-steps of the score product
  constexpr int NB = DK / 16;  // 16-wide blocks of d in the output
  __shared__ __attribute__((aligned(16))) uint16_t vt[DK * kFsVtLd];
  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int len = min(max(lens[b], 0), T);
  const int q0 = blockIdx.x * (kFsMhaWaves * 16) + wave * 16;
  const int qrow = min(q0 + c, T - 1);  // a row past the end repeats the last one and is not stored
  const uint16_t* qp = q + ((int64_t)b * rows_in + qrow) * ldq + h * DK + g * 8;
  const uint16_t* kb = k + (int64_t)b * rows_in * ldk + h * DK + g * 8;
  const uint16_t* vb = v + (int64_t)b * rows_in * ldv + h * DK;
  bf16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
  f32x4 o[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) o[n] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  float m = -INFINITY, l = 0.0f;  // l: this lane's share of the sum (the four lanes of a query are added at the end)

  for (int kt = 0; kt < len; kt += kFsKeyTile) {
    // stage V^T: chunk = 8 d of one key; a masked key is staged as zeros whatever its row holds
    for (int i = tid; i < kFsKeyTile * (DK / 8); i += kFsMhaWaves * 64) {
      const int key = i / (DK / 8), d0 = (i % (DK / 8)) * 8;
      u32x4 w = {0u, 0u, 0u, 0u};
      if (kt + key < len) w = *reinterpret_cast<const u32x4*>(vb + (int64_t)(kt + key) * ldv + d0);
      const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vt[(d0 + 2 * e) * kFsVtLd + key] = (uint16_t)(ws[e] & 0xffffu);
        vt[(d0 + 2 * e + 1) * kFsVtLd + key] = (uint16_t)(ws[e] >> 16);
      }
    }
    __syncthreads();
    f32x4 s[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      s[sub] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
      const int krow = min(kt + 16 * sub + c, T - 1);
      const uint16_t* kp = kb + (int64_t)krow * ldk;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        s[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kp + ks * 32), qf[ks], s[sub], 0, 0, 0);
    }
    // s[sub][r]: key kt + 16 sub + 4 g + r against query c
    float sv[8];
    bool ok[8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = kt + 16 * (j >> 2) + 4 * g + (j & 3);
      ok[j] = key < len;
      sv[j] = s[j >> 2][j & 3] * scale;
      if (ok[j]) mx = fmaxf(mx, sv[j]);
    }
    mx = max_xor32(max_xor16(mx));  // finite: key kt is valid
    const float m_new = fmaxf(m, mx);
    const float alpha = __expf(m - m_new);
    m = m_new;
    float p[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = ok[j] ? __expf(sv[j] - m_new) : 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j += 2) bf16_round2(p[j], p[j + 1]);  // the weights that multiply V are the ones that are summed
    l = l * alpha + (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])));
    const u32x4 pw = {pack2_bf16(p[0], p[1]), pack2_bf16(p[2], p[3]), pack2_bf16(p[4], p[5]), pack2_bf16(p[6], p[7])};
    const bf16x8 pb = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      o[n] *= alpha;
      const uint16_t* vr = vt + (16 * n + c) * kFsVtLd + 4 * g;
      const uint2 lo = *reinterpret_cast<const uint2*>(vr), hi = *reinterpret_cast<const uint2*>(vr + 16);
      const u32x4 vw = {lo.x, lo.y, hi.x, hi.y};
      o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vw), pb, o[n], 0, 0, 0);
    }
    __syncthreads();
  }
  l = sum_xor32(sum_xor16(l));
  const float inv = l > 0.0f ? 1.0f / l : 0.0f;  // no valid key: the row is written as zeros
  if (q0 + c < T) {
    uint16_t* op = ctx + ((int64_t)b * rows_out + q0 + c) * ldc + h * DK + 4 * g;
#pragma unroll
    for (int n = 0; n < NB; ++n)  // o[n][r]: d = 16 n + 4 g + r of query c
      *reinterpret_cast<uint2*>(op + 16 * n) = make_uint2(pack2_bf16(o[n].x * inv, o[n].y * inv), pack2_bf16(o[n].z * inv, o[n].w * inv));
  }
}

// ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------
// thread -> (row r0 + i * rpp, channels 4 cq .. 4 cq + 3); all four channels lie in one group (C / G % 4 == 0)
__global__ __launch_bounds__(kFsThreads) void fs2_gn_stats_kernel(const float* __restrict__ x, int T, int C, int G, double* __restrict__ part) {
  __shared__ double red[kFsThreads];
  __shared__ double mean_s[64];
  const int tid = threadIdx.x, tpr = C >> 2, rpp = kFsThreads / tpr, cq = tid % tpr, r0 = tid / tpr;
  const int cg = C / G, grp = (cq * 4) / cg;
  const int t0 = blockIdx.x * kFsStatRows, t1 = min(T, t0 + kFsStatRows);
  const float* xb = x + (int64_t)blockIdx.y * T * C + cq * 4;
  const double n = (double)(t1 - t0) * cg;
  double acc = 0.0;
  for (int t = t0 + r0; t < t1; t += rpp) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(xb + (int64_t)t * C);
    acc += ((double)a.x + (double)a.y) + ((double)a.z + (double)a.w);
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < G) {
    double sum = 0.0;
    for (int j = 0; j < kFsThreads; ++j)
      if (((j % tpr) * 4) / cg == tid) sum += red[j];
    mean_s[tid] = sum / n;
  }
  __syncthreads();
  const double mean = mean_s[grp];
  acc = 0.0;
  for (int t = t0 + r0; t < t1; t += rpp) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(xb + (int64_t)t * C);
    const double d0 = a.x - mean, d1 = a.y - mean, d2 = a.z - mean, d3 = a.w - mean;
    acc += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  __syncthreads();
  red[tid] = acc;
  __syncthreads();
  if (tid < G) {
    double sum = 0.0;
    for (int j = 0; j < kFsThreads; ++j)
      if (((j % tpr) * 4) / cg == tid) sum += red[j];
    double* o = part + (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * G + tid) * 2;
    o[0] = mean_s[tid];
    o[1] = sum;
  }
}

__global__ __launch_bounds__(kFsThreads) void fs2_gn_apply_kernel(const float* __restrict__ x, int T, int C, int Cpad, int G, int halo,
                                                                  const double* __restrict__ part, int parts, float eps,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const int32_t* __restrict__ lens, float* __restrict__ out,
                                                                  uint16_t* __restrict__ img) {
  __shared__ double mean_s[64], rstd_s[64];
  const int tid = threadIdx.x, b = blockIdx.y, cg = C / G;
  if (tid < G) {  // the partials in part order
    double na = 0.0, mean = 0.0, m2 = 0.0;
    for (int p = 0; p < parts; ++p) {
      const double* pp = part + (((int64_t)b * parts + p) * G + tid) * 2;
      const double nb = (double)(min(T, (p + 1) * kFsStatRows) - p * kFsStatRows) * cg;
      const double delta = pp[0] - mean, nn = na + nb;
      mean += delta * (nb / nn);
      m2 += pp[1] + delta * delta * (na * nb / nn);
      na = nn;
    }
    mean_s[tid] = mean;
    rstd_s[tid] = 1.0 / sqrt(m2 / na + (double)eps);
  }
  __syncthreads();
  const int c8n = Cpad >> 3, rows_u = T + 2 * halo;
  const int64_t idx = (int64_t)blockIdx.x * kFsThreads + tid;
  if (idx >= (int64_t)rows_u * c8n) return;
  const int c = (int)(idx % c8n) * 8, t = (int)(idx / c8n) - halo;
  const int len = lens ? lens[b] : T;
  u32x4 ob = {0u, 0u, 0u, 0u};
  if (t >= 0 && t < T && c < C) {
    float y[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int64_t off = ((int64_t)b * T + t) * C + c;
    if (t < len) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(x + off), x1 = *reinterpret_cast<const f32x4*>(x + off + 4);
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c), g1 = *reinterpret_cast<const f32x4*>(gamma + c + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + c), b1 = *reinterpret_cast<const f32x4*>(beta + c + 4);
      const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int grp = (c + i) / cg;
        y[i] = fmaf((float)(((double)xv[i] - mean_s[grp]) * rstd_s[grp]), gv[i], bv[i]);
      }
    }
    if (out) {
      *reinterpret_cast<f32x4*>(out + off) = (f32x4){y[0], y[1], y[2], y[3]};
      *reinterpret_cast<f32x4*>(out + off + 4) = (f32x4){y[4], y[5], y[6], y[7]};
    }
    ob = (u32x4){pack2_bf16(y[0], y[1]), pack2_bf16(y[2], y[3]), pack2_bf16(y[4], y[5]), pack2_bf16(y[6], y[7])};
  }
  if (img) *reinterpret_cast<u32x4*>(img + (((int64_t)b * rows_u + t + halo) * Cpad + c)) = ob;
}

// ---- one row per wave ------------------------------------------------------------------------------------------------------------------
constexpr int kFsRowMax = 16;  // floats of a row per lane: rows up to 1024 wide

// v[i] = element lane + 64 i of the row (i < ne); -> normalised, scaled and shifted in place
__device__ __forceinline__ void fs2_row_layernorm(float (&v)[kFsRowMax], int ne, int lane, int F, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps) {
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < kFsRowMax; ++i)
    if (i < ne) s += v[i];
  const float mean = wave_sum(s) / (float)F;
  float s2 = 0.0f;
#pragma unroll
  for (int i = 0; i < kFsRowMax; ++i)
    if (i < ne) {
      const float d = v[i] - mean;
      s2 = fmaf(d, d, s2);
    }
  const float rstd = 1.0f / sqrtf(wave_sum(s2) / (float)F + eps);
#pragma unroll
  for (int i = 0; i < kFsRowMax; ++i)
    if (i < ne) v[i] = fmaf((v[i] - mean) * rstd, gamma[lane + 64 * i], beta[lane + 64 * i]);
}

__global__ __launch_bounds__(kFsThreads) void fs2_rowln_kernel(const float* __restrict__ x, int64_t B, int T, int F, int halo,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               const int32_t* __restrict__ lens, float* __restrict__ out,
                                                               uint16_t* __restrict__ img) {
  const int lane = threadIdx.x & 63, rows_u = T + 2 * halo, ne = F >> 6;
  const int64_t row = (int64_t)blockIdx.x * (kFsThreads / 64) + (threadIdx.x >> 6);
  if (row >= B * rows_u) return;
  const int64_t b = row / rows_u;
  const int t = (int)(row - b * rows_u) - halo;
  float v[kFsRowMax];
#pragma unroll
  for (int i = 0; i < kFsRowMax; ++i) v[i] = 0.0f;
  const bool real = t >= 0 && t < T;
  if (real && (!lens || t < lens[b])) {
    const float* xr = x + (b * T + t) * F;
#pragma unroll
    for (int i = 0; i < kFsRowMax; ++i)
      if (i < ne) v[i] = xr[lane + 64 * i];
    fs2_row_layernorm(v, ne, lane, F, gamma, beta, eps);
  }
#pragma unroll
  for (int i = 0; i < kFsRowMax; ++i)
    if (i < ne) {
      if (out && real) out[(b * T + t) * F + lane + 64 * i] = v[i];
      if (img) img[row * F + lane + 64 * i] = f2bf(v[i]);
    }
}

__global__ __launch_bounds__(kFsThreads) void fs2_head_kernel(const float* __restrict__ hid, int64_t B, int T, int F, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, const float* __restrict__ w,
                                                              const float* __restrict__ bias, const int32_t* __restrict__ lens, float control,
                                                              float* __restrict__ pred, const float* __restrict__ bins, int n_bins,
                                                              const int32_t* __restrict__ index_in, int32_t* __restrict__ index_out,
                                                              const float* __restrict__ table, const float* __restrict__ x,
                                                              const float* __restrict__ pos, int C, int halo, float* __restrict__ x_out,
                                                              float* __restrict__ x_pos, uint16_t* __restrict__ img) {
  const int lane = threadIdx.x & 63, rows_u = T + 2 * halo, ne = F >> 6;
  const int64_t row = (int64_t)blockIdx.x * (kFsThreads / 64) + (threadIdx.x >> 6);
  if (row >= B * rows_u) return;
  const int64_t b = row / rows_u;
  const int t = (int)(row - b * rows_u) - halo;
  if (t < 0 || t >= T) {  // a halo row of the operand image
    if (img)
      for (int c = lane; c < C; c += 64) img[row * C + c] = 0;
    return;
  }
  const int64_t r = b * T + t;
  float v[kFsRowMax];
#pragma unroll
  for (int i = 0; i < kFsRowMax; ++i) v[i] = i < ne ? hid[r * F + lane + 64 * i] : 0.0f;
  fs2_row_layernorm(v, ne, lane, F, gamma, beta, eps);
  float d = 0.0f;
#pragma unroll
  for (int i = 0; i < kFsRowMax; ++i)
    if (i < ne) d = fmaf(v[i], w[lane + 64 * i], d);
  float val = wave_sum(d) + bias[0];
  if (lens && t >= lens[b]) val *= 0.0f;  // x * (1 - mask), variance_adapter.py:84-87
  val *= control;
  if (lane == 0) pred[r] = val;
  if (!table) return;
  int idx = 0;
  if (index_in) {
    idx = min(max(index_in[r], 0), n_bins - 1);
  } else {
    for (int j0 = 0; j0 < n_bins - 1; j0 += 64) {  // #{bins < val}: searchsorted, side left
      const int j = j0 + lane;
      idx += __popcll(__ballot(j < n_bins - 1 && bins[j] < val));
    }
  }
  if (index_out && lane == 0) index_out[r] = idx;
  for (int c = lane; c < C; c += 64) {
    float y = x[r * C + c] + table[(int64_t)idx * C + c];
    if (x_out) x_out[r * C + c] = y;
    if (pos) y += pos[(int64_t)t * C + c];
    if (x_pos) x_pos[r * C + c] = y;
    if (img) img[row * C + c] = f2bf(y);
  }
}

__global__ __launch_bounds__(kFsThreads) void fs2_embed_kernel(const int32_t* __restrict__ ids, int T, int C, int V, int halo,
                                                               const float* __restrict__ table, const float* __restrict__ pos,
                                                               float* __restrict__ out, uint16_t* __restrict__ img, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
  if (idx >= total) return;
  const int c8n = C >> 3, rows_u = T + 2 * halo;
  const int c = (int)(idx % c8n) * 8;
  const int64_t row = idx / c8n, b = row / rows_u;
  const int t = (int)(row - b * rows_u) - halo;
  u32x4 ob = {0u, 0u, 0u, 0u};
  if (t >= 0 && t < T) {
    const int id = ids[b * T + t];
    float y[8];
    const float* pp = pos + (int64_t)t * C + c;
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = pp[i];
    if (id >= 0 && id < V) {  // an id outside the table adds nothing
      const float* tp = table + (int64_t)id * C + c;
#pragma unroll
      for (int i = 0; i < 8; ++i) y[i] = tp[i] + y[i];
    }
    float* o = out + (b * T + t) * C + c;
    *reinterpret_cast<f32x4*>(o) = (f32x4){y[0], y[1], y[2], y[3]};
    *reinterpret_cast<f32x4*>(o + 4) = (f32x4){y[4], y[5], y[6], y[7]};
    ob = (u32x4){pack2_bf16(y[0], y[1]), pack2_bf16(y[2], y[3]), pack2_bf16(y[4], y[5]), pack2_bf16(y[6], y[7])};
  }
  if (img) *reinterpret_cast<u32x4*>(img + row * C + c) = ob;
}

// round(exp(logd) - 1) * d_control, clipped at 0 (variance_adapter.py:290-291).  exp through float64 and one rounding (the correctly
// rounded float32 exp but for ties the float64 result cannot show); the subtraction and the product are single float32 operations.
__global__ __launch_bounds__(kFsThreads) void fs2_duration_kernel(const float* __restrict__ logd, int64_t n, float d_control,
                                                                  float* __restrict__ dur) {
  const int64_t i = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
  if (i >= n) return;
  const float e = (float)exp((double)logd[i]);
  const float r = rintf(__fsub_rn(e, 1.0f));  // round half to even, as ms.ops.round
  dur[i] = fmaxf(__fmul_rn(r, d_control), 0.0f);
}

__global__ __launch_bounds__(kFsThreads) void fs2_length_regulate_kernel(const float* __restrict__ dur, const int32_t* __restrict__ ids, int Ts,
                                                                         int32_t* __restrict__ prefix, int32_t* __restrict__ mel_len,
                                                                         int32_t* __restrict__ expanded, int Tcap) {
  __shared__ int32_t pre[kFsMaxSrc];
  __shared__ int32_t part[kFsThreads + 1];
  const int tid = threadIdx.x, b = blockIdx.x, chunk = (Ts + kFsThreads - 1) / kFsThreads;
  const int i0 = min(tid * chunk, Ts), i1 = min(i0 + chunk, Ts);
  const float* db = dur + (int64_t)b * Ts;
  int32_t sum = 0;
  for (int i = i0; i < i1; ++i) {
    const float d = db[i];
    const int32_t di = d > 0.0f ? (int32_t)fminf(d, (float)kFsMaxDur) : 0;  // truncation, as .astype(np.int32) (a NaN counts as 0)
    pre[i] = di;
    sum += di;
  }
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int32_t run = 0;
    for (int j = 0; j < kFsThreads; ++j) {
      const int32_t s = part[j];
      part[j] = run;
      run += s;
    }
    part[kFsThreads] = run;
    mel_len[b] = run;
  }
  __syncthreads();
  int32_t run = part[tid];
  for (int i = i0; i < i1; ++i) {
    const int32_t di = pre[i];
    pre[i] = run;
    if (prefix) prefix[(int64_t)b * Ts + i] = run;
    run += di;
  }
  __syncthreads();
  if (!expanded) return;
  const int32_t total = part[kFsThreads];
  for (int t = tid; t < Tcap; t += kFsThreads) {
    int32_t id = 0;  // PAD
    if (t < total) {
      int lo = 0, hi = Ts;  // the last i with pre[i] <= t: phonemes of duration 0 share their successor's prefix and are skipped
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= t) lo = mid; else hi = mid;
      }
      id = ids[(int64_t)b * Ts + lo];
    }
    expanded[(int64_t)b * Tcap + t] = id;
  }
}

static inline bool fs2_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static inline int64_t fs2_up(int64_t n) { return (n + 255) / 256 * 256; }

struct Fs2Layout {  // byte offsets of a stack's workspace
  int64_t qkv, ctx, y, hid, part, total;
  int parts;
};

static int fs2_layout(const ma_fs2_plan_t* pl, Fs2Layout& L) {
  if (!pl || !pl->layers || pl->n_layers < 1 || pl->B < 1 || pl->T < 1 || pl->heads < 1 || pl->d_model < 1 || pl->d_inner < 1 || pl->halo < 0 ||
      pl->groups < 0 || pl->k1 < 1 || !(pl->k1 & 1))
    return MA_ERR_INVALID_ARG;
  const int C = pl->d_model;
  if (C % pl->heads) return MA_ERR_INVALID_ARG;
  const int dk = C / pl->heads;
  if ((dk != 32 && dk != 64 && dk != 128) || (C & 63) || C > 1024 || (pl->d_inner & 63) || pl->B > 65535 || pl->T > (1 << 20)) return MA_ERR_UNSUPPORTED;
  if (pl->halo < pl->k1 / 2) return MA_ERR_INVALID_ARG;  // a tap would read the neighbouring utterance
  if (pl->groups > 0 && (pl->groups > 64 || C % pl->groups || (C / pl->groups) % 4 || kFsThreads % (C / 4))) return MA_ERR_UNSUPPORTED;
  const int64_t B = pl->B, T = pl->T, rows_u = T + 2 * (int64_t)pl->halo;
  L.parts = (int)((T + kFsStatRows - 1) / kFsStatRows);
  L.qkv = 0;
  L.ctx = L.qkv + fs2_up(B * rows_u * 3 * C * 2);
  L.y = L.ctx + fs2_up(B * T * C * 2);
  L.hid = L.y + fs2_up(B * T * C * 4);
  L.part = L.hid + fs2_up(B * T * pl->d_inner * 2);
  L.total = L.part + fs2_up(B * L.parts * 64 * 2 * 8);
  return MA_OK;
}

}  // namespace ma

using namespace ma;

extern "C" {

int ma_mha_d128_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const int32_t* lens, int64_t B,
                     int64_t T, int64_t rows_in, int32_t H, int32_t d_k, float scale, void* ctx, int64_t ldc, int64_t rows_out,
                     ma_stream_t stream) {
  if (!q || !k || !v || !lens || !ctx || B < 1 || T < 1 || H < 1 || rows_in < T || rows_out < T) return MA_ERR_INVALID_ARG;
  if (ldq < (int64_t)H * d_k || ldk < (int64_t)H * d_k || ldv < (int64_t)H * d_k || ldc < (int64_t)H * d_k) return MA_ERR_INVALID_ARG;
  if (fs2_misaligned(q) || fs2_misaligned(k) || fs2_misaligned(v) || fs2_misaligned(ctx)) return MA_ERR_INVALID_ARG;
  if ((d_k != 32 && d_k != 64 && d_k != 128) || (ldq & 7) || (ldk & 7) || (ldv & 7) || (ldc & 7) || B > 65535 || H > 65535 || T > (1 << 20))
    return MA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((T + kFsMhaWaves * 16 - 1) / (kFsMhaWaves * 16)), (unsigned)H, (unsigned)B), block(kFsMhaWaves * 64);
  const uint16_t *qp = (const uint16_t*)q, *kp = (const uint16_t*)k, *vp = (const uint16_t*)v;
  if (d_k == 128)
    MA_LAUNCH(fs2_mha_kernel<128>, grid, block, 0, (hipStream_t)stream, qp, kp, vp, ldq, ldk, ldv, lens, (int)T, rows_in, scale, (uint16_t*)ctx, ldc, rows_out);
  else if (d_k == 64)
    MA_LAUNCH(fs2_mha_kernel<64>, grid, block, 0, (hipStream_t)stream, qp, kp, vp, ldq, ldk, ldv, lens, (int)T, rows_in, scale, (uint16_t*)ctx, ldc, rows_out);
  else
    MA_LAUNCH(fs2_mha_kernel<32>, grid, block, 0, (hipStream_t)stream, qp, kp, vp, ldq, ldk, ldv, lens, (int)T, rows_in, scale, (uint16_t*)ctx, ldc, rows_out);
  return MA_OK;
}

int32_t ma_groupnorm_parts(int64_t T) { return T < 1 || T > (1 << 20) ? MA_ERR_INVALID_ARG : (int32_t)((T + kFsStatRows - 1) / kFsStatRows); }

int ma_groupnorm_stats(const float* x, int64_t B, int64_t T, int32_t C, int32_t G, double* part, ma_stream_t stream) {
  if (!x || !part || B < 1 || T < 1 || C < 1 || G < 1 || fs2_misaligned(x) || (reinterpret_cast<uintptr_t>(part) & 7)) return MA_ERR_INVALID_ARG;
  if (G > 64 || C % G || (C / G) % 4 || C > 1024 || kFsThreads % (C / 4) || B > 65535 || T > (1 << 20)) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(fs2_gn_stats_kernel, dim3((unsigned)ma_groupnorm_parts(T), (unsigned)B), dim3(kFsThreads), 0, (hipStream_t)stream, x, (int)T, C, G, part);
  return MA_OK;
}

int ma_groupnorm_apply(const float* x, int64_t B, int64_t T, int32_t C, int32_t Cpad, int32_t G, int32_t halo, const double* part, float eps,
                       const float* gamma, const float* beta, const int32_t* lens, float* out, void* img, ma_stream_t stream) {
  if (!x || !part || !gamma || !beta || (!out && !img) || B < 1 || T < 1 || C < 1 || G < 1 || halo < 0 || Cpad < C) return MA_ERR_INVALID_ARG;
  if (fs2_misaligned(x) || fs2_misaligned(gamma) || fs2_misaligned(beta) || fs2_misaligned(out) || fs2_misaligned(img)) return MA_ERR_INVALID_ARG;
  if (G > 64 || C % G || (C & 7) || (Cpad & 7) || B > 65535 || T > (1 << 20)) return MA_ERR_UNSUPPORTED;
  const int64_t total = (T + 2 * (int64_t)halo) * (Cpad >> 3), blocks = (total + kFsThreads - 1) / kFsThreads;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(fs2_gn_apply_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(kFsThreads), 0, (hipStream_t)stream, x, (int)T, C, Cpad, G, halo, part,
            (int)ma_groupnorm_parts(T), eps, gamma, beta, lens, out, (uint16_t*)img);
  return MA_OK;
}

int ma_fs2_layernorm_pack_f32(const float* x, int64_t B, int64_t T, int32_t F, int32_t halo, const float* gamma, const float* beta, float eps,
                              const int32_t* lens, float* out, void* img, ma_stream_t stream) {
  if (!x || !gamma || !beta || (!out && !img) || B < 1 || T < 1 || F < 1 || halo < 0) return MA_ERR_INVALID_ARG;
  if ((F & 63) || F > 64 * kFsRowMax || T > (1 << 20)) return MA_ERR_UNSUPPORTED;
  const int64_t rows = B * (T + 2 * (int64_t)halo), blocks = (rows + 3) / 4;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(fs2_rowln_kernel, dim3((unsigned)blocks), dim3(kFsThreads), 0, (hipStream_t)stream, x, B, (int)T, F, halo, gamma, beta, eps, lens, out,
            (uint16_t*)img);
  return MA_OK;
}

int ma_variance_head_f32(const float* hid, int64_t B, int64_t T, int32_t F, const float* gamma, const float* beta, float eps, const float* w,
                         const float* bias, const int32_t* lens, float control, float* pred, const float* bins, int32_t n_bins,
                         const int32_t* index_in, int32_t* index_out, const float* table, const float* x, const float* pos, int32_t C,
                         int32_t halo, float* x_out, float* x_pos, void* img, ma_stream_t stream) {
  if (!hid || !gamma || !beta || !w || !bias || !pred || B < 1 || T < 1 || F < 1 || halo < 0) return MA_ERR_INVALID_ARG;
  if (table && (!x || (!bins && !index_in) || n_bins < 2 || C < 1 || (!x_out && !x_pos && !img) || (x_pos && !pos))) return MA_ERR_INVALID_ARG;
  if ((F & 63) || F > 64 * kFsRowMax || T > (1 << 20)) return MA_ERR_UNSUPPORTED;
  const int h = table && img ? halo : 0;
  const int64_t rows = B * (T + 2 * (int64_t)h), blocks = (rows + 3) / 4;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(fs2_head_kernel, dim3((unsigned)blocks), dim3(kFsThreads), 0, (hipStream_t)stream, hid, B, (int)T, F, gamma, beta, eps, w, bias, lens,
            control, pred, bins, n_bins, index_in, index_out, table, x, pos, C, h, x_out, x_pos, table ? (uint16_t*)img : nullptr);
  return MA_OK;
}

int ma_fs2_embed_f32(const int32_t* ids, int64_t B, int64_t T, int32_t C, int32_t V, int32_t halo, const float* table, const float* pos,
                     float* out, void* img, ma_stream_t stream) {
  if (!ids || !table || !pos || !out || B < 1 || T < 1 || C < 1 || V < 1 || halo < 0) return MA_ERR_INVALID_ARG;
  if (fs2_misaligned(out) || fs2_misaligned(img)) return MA_ERR_INVALID_ARG;
  if ((C & 7) || T > (1 << 20)) return MA_ERR_UNSUPPORTED;
  const int64_t total = B * (T + 2 * (int64_t)halo) * (C >> 3), blocks = (total + kFsThreads - 1) / kFsThreads;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(fs2_embed_kernel, dim3((unsigned)blocks), dim3(kFsThreads), 0, (hipStream_t)stream, ids, (int)T, C, V, halo, table, pos, out,
            (uint16_t*)img, total);
  return MA_OK;
}

int ma_fs2_durations_f32(const float* logd, int64_t n, float d_control, float* dur, ma_stream_t stream) {
  if (!logd || !dur || n < 1) return MA_ERR_INVALID_ARG;
  const int64_t blocks = (n + kFsThreads - 1) / kFsThreads;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(fs2_duration_kernel, dim3((unsigned)blocks), dim3(kFsThreads), 0, (hipStream_t)stream, logd, n, d_control, dur);
  return MA_OK;
}

int ma_length_regulate_i32(const float* dur, const int32_t* ids, int64_t B, int32_t T_src, int32_t* prefix, int32_t* mel_len,
                           int32_t* expanded, int32_t T_cap, ma_stream_t stream) {
  if (!dur || !mel_len || B < 1 || T_src < 1 || (expanded && (!ids || T_cap < 1))) return MA_ERR_INVALID_ARG;
  if (T_src > kFsMaxSrc || B > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(fs2_length_regulate_kernel, dim3((unsigned)B), dim3(kFsThreads), 0, (hipStream_t)stream, dur, ids, T_src, prefix, mel_len, expanded,
            T_cap);
  return MA_OK;
}

int64_t ma_fs2_workspace_bytes(const ma_fs2_plan_t* plan) {
  Fs2Layout L;
  const int rc = fs2_layout(plan, L);
  return rc != MA_OK ? rc : L.total;
}

int ma_fs2_fft_stack(const ma_fs2_plan_t* plan, float* x, void* img, const int32_t* lens, void* workspace, int64_t workspace_bytes,
                     ma_stream_t stream) {
  Fs2Layout L;
  int rc = fs2_layout(plan, L);
  if (rc != MA_OK) return rc;
  if (!x || !img || !lens || !workspace || fs2_misaligned(x) || fs2_misaligned(img) || fs2_misaligned(workspace)) return MA_ERR_INVALID_ARG;
  if (workspace_bytes < L.total) return MA_ERR_WORKSPACE;
  for (int i = 0; i < plan->n_layers; ++i) {  // every layer before the first launch
    const ma_fs2_layer_t& ly = plan->layers[i];
    if (!ly.w_qkv || !ly.b_qkv || !ly.w_fc || !ly.b_fc || !ly.w_1 || !ly.b_1 || !ly.w_2 || !ly.b_2 || !ly.gamma1 || !ly.beta1 || !ly.gamma2 ||
        !ly.beta2)
      return MA_ERR_INVALID_ARG;
  }
  const int64_t B = plan->B, T = plan->T, rows_u = T + 2 * (int64_t)plan->halo;
  const int C = plan->d_model, H = plan->heads, dk = C / H, D = plan->d_inner, halo = plan->halo;
  char* ws = static_cast<char*>(workspace);
  uint16_t* qkv = reinterpret_cast<uint16_t*>(ws + L.qkv);
  uint16_t* ctx = reinterpret_cast<uint16_t*>(ws + L.ctx);
  float* y = reinterpret_cast<float*>(ws + L.y);
  uint16_t* hid = reinterpret_cast<uint16_t*>(ws + L.hid);
  double* part = reinterpret_cast<double*>(ws + L.part);
  uint16_t* xb = static_cast<uint16_t*>(img);
  const float scale = 1.0f / sqrtf((float)dk);  // attn / temperature, temperature = d_k ** 0.5 (sublayers.py:53-55)
  auto norm = [&](const float* g, const float* be) -> int {  // y -> x, img
    if (plan->groups == 0) return ma_fs2_layernorm_pack_f32(y, B, T, C, halo, g, be, plan->eps, lens, x, xb, stream);
    const int r = ma_groupnorm_stats(y, B, T, C, plan->groups, part, stream);
    if (r != MA_OK) return r;
    return ma_groupnorm_apply(y, B, T, C, C, plan->groups, halo, part, plan->eps, g, be, lens, x, xb, stream);
  };
  for (int i = 0; i < plan->n_layers; ++i) {
    const ma_fs2_layer_t& ly = plan->layers[i];
    ma_gemm_epilogue_t e = {};
    e.alpha = 1.0f;
    e.bias = ly.b_qkv;
    e.out_bf16 = 1;
    rc = ma_gemm_bf16(xb, C, ly.w_qkv, C, qkv, 3 * C, B * rows_u, 3 * C, C, &e, stream);  // halo rows come out as the bias and are never read
    if (rc != MA_OK) return rc;
    const uint16_t* q0 = qkv + (int64_t)halo * 3 * C;
    rc = ma_mha_d128_bf16(q0, 3 * C, q0 + C, 3 * C, q0 + 2 * C, 3 * C, lens, B, T, rows_u, H, dk, scale, ctx, C, T, stream);
    if (rc != MA_OK) return rc;
    e = ma_gemm_epilogue_t{};
    e.alpha = 1.0f;
    e.bias = ly.b_fc;
    e.residual = x;
    e.ldr = C;
    rc = ma_gemm_bf16(ctx, C, ly.w_fc, C, y, C, B * T, C, C, &e, stream);
    if (rc != MA_OK) return rc;
    rc = norm(ly.gamma1, ly.beta1);
    if (rc != MA_OK) return rc;
    e = ma_gemm_epilogue_t{};
    e.alpha = 1.0f;
    e.bias = ly.b_1;
    e.act = 2;
    e.out_bf16 = 1;
    for (int64_t b = 0; b < B; ++b) {  // one product per utterance: its halo rows are the convolution's zero padding
      rc = ma_conv1d_taps_bf16(xb + (b * rows_u + halo) * C, C, T, C, plan->k1, 1, ly.w_1, hid + b * T * D, D, D, &e, stream);
      if (rc != MA_OK) return rc;
    }
    e = ma_gemm_epilogue_t{};
    e.alpha = 1.0f;
    e.bias = ly.b_2;
    e.residual = x;
    e.ldr = C;
    rc = ma_gemm_bf16(hid, D, ly.w_2, D, y, C, B * T, C, D, &e, stream);
    if (rc != MA_OK) return rc;
    rc = norm(ly.gamma2, ly.beta2);
    if (rc != MA_OK) return rc;
  }
  return MA_OK;
}

}  // extern "C"
