// Conv-TasNet training (examples/conv_tasnet/train.py around mindaudio/models/conv_tasnet.py and separation_loss.py): what the
// backward needs besides the GEMMs.  Contract: include/mindaudio_amd.h.
//
// Layout and statistics as conv_tasnet.hip: (M * K, channels) float32 activations, utterance m in the rows [m * K, (m + 1) * K), a tile
// of 8192 / C rows per workgroup, float64 partials per tile that the CONSUMER joins in index order.  The backward of a global layer
// norm needs two more whole-utterance sums, sum(dy) and sum(dy * xhat); they travel the same way, two float64 per tile.  xhat is never
// stored: it is recomputed from the saved pre-activation, the PReLU slope and the forward's moments.
//
// Parameter gradients (PReLU slopes, depthwise taps, basis signals, encoder filters) leave as one float32 partial per workgroup; the
// caller sums them in a fixed order with ma_reduce_splits_batch_f32.  No atomics anywhere: the same bits from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"
#include "tasnet_common.h"

namespace ma {

// mean(dy) and mean(dy * xhat) of an utterance from its (sum, sum) partials; `count` = K * C
__device__ __forceinline__ void gln_bwd_means(const double* __restrict__ part2, int nparts, double count, double* sh, double& m1,
                                              double& m2) {
  if (threadIdx.x < 64) {
    double a = 0.0, b = 0.0;
    for (int p = threadIdx.x; p < nparts; p += 64) {
      a += part2[2 * p];
      b += part2[2 * p + 1];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (threadIdx.x == 0) {
      sh[0] = a / count;
      sh[1] = b / count;
    }
  }
  __syncthreads();
  m1 = sh[0];
  m2 = sh[1];
  __syncthreads();
}

// The statistics of one gLN backward.  The activation gradients use the float32 values; a PReLU slope's gradient is ONE number summed
// over a whole tensor with cancelling signs, so its terms are formed in float64 from the float64 statistics (in float32 their rounding
// alone moved the sum by 1.5e-6 of its value).
struct GlnBwd {
  float mean, rstd, m1, m2;
  double mean_d, rstd_d, m1_d, m2_d;
};
__device__ __forceinline__ GlnBwd gln_bwd_load(const double* __restrict__ part, const double* __restrict__ part2, int nparts,
                                               double count, double* sh) {
  GlnBwd s;
  gln_mean_rstd_f64(part, nparts, sh, s.mean_d, s.rstd_d);
  gln_bwd_means(part2, nparts, count, sh, s.m1_d, s.m2_d);
  s.mean = (float)s.mean_d;
  s.rstd = (float)s.rstd_d;
  s.m1 = (float)s.m1_d;
  s.m2 = (float)s.m2_d;
  return s;
}
// dz * pre of an element on the negative side, in float64
__device__ __forceinline__ double slope_term(float dy, float pre, float a, const GlnBwd& s) {
  const double xh = ((double)(a * pre) - s.mean_d) * s.rstd_d;
  return ((double)dy - s.m1_d - xh * s.m2_d) * s.rstd_d * (double)pre;
}

struct TileGeom {
  int64_t m, row0, base;
  int rows_here, C4, n4;
};
__device__ __forceinline__ TileGeom tile_geom(int64_t K, int C, int rows) {
  TileGeom g;
  g.m = blockIdx.y;
  g.row0 = (int64_t)blockIdx.x * rows;
  g.rows_here = K - g.row0 < rows ? (int)(K - g.row0) : rows;
  g.C4 = C / 4;
  g.n4 = g.rows_here * g.C4;
  g.base = (g.m * K + g.row0) * C;
  return g;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float comp(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ float& comp(float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// ---- training forward: ma_gln_dwconv_prelu that also keeps the depthwise output BEFORE its PReLU ----------------------------------------
__global__ __launch_bounds__(kTnThreads) void gln_dwconv_prelu_train_kernel(const float* __restrict__ y, int64_t K, int C, int rows,
                                                                            const double* __restrict__ part_in, int nparts_in,
                                                                            const float* __restrict__ Wt, int dil,
                                                                            const float* __restrict__ a_ptr, float* __restrict__ pre,
                                                                            float* __restrict__ z, double* __restrict__ part) {
  __shared__ double sh[4];
  const TileGeom g = tile_geom(K, C, rows);
  float mean, rstd;
  gln_mean_rstd(part_in + g.m * nparts_in * 3, nparts_in, sh, mean, rstd);
  const float a = a_ptr[0];
  const int64_t step = (int64_t)dil * C;
  float4 v[kTnIter4];
  double ts = 0.0;
#pragma unroll
  for (int i = 0; i < kTnIter4; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (e < g.n4) {
      const int r = e / g.C4, c = (e - r * g.C4) * 4;
      const int64_t k = g.row0 + r;
      const float* p = y + g.base + (int64_t)e * 4;
      const float4 w0 = ld4(Wt + c), w1 = ld4(Wt + C + c), w2 = ld4(Wt + 2 * C + c);
      float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (k - dil >= 0) {
        const float4 q = ld4(p - step);
#pragma unroll
        for (int j = 0; j < 4; ++j) comp(t, j) = comp(w0, j) * ((comp(q, j) - mean) * rstd);
      }
      {
        const float4 q = ld4(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) comp(t, j) = fmaf(comp(w1, j), (comp(q, j) - mean) * rstd, comp(t, j));
      }
      if (k + dil < K) {
        const float4 q = ld4(p + step);
#pragma unroll
        for (int j = 0; j < 4; ++j) comp(t, j) = fmaf(comp(w2, j), (comp(q, j) - mean) * rstd, comp(t, j));
      }
      *reinterpret_cast<float4*>(pre + g.base + (int64_t)e * 4) = t;
#pragma unroll
      for (int j = 0; j < 4; ++j) comp(t, j) = prelu(comp(t, j), a);
      *reinterpret_cast<float4*>(z + g.base + (int64_t)e * 4) = t;
      v[i] = t;
      ts += ((double)t.x + (double)t.y) + ((double)t.z + (double)t.w);
    }
  }
  tile_moments(ts, (int64_t)g.n4 * 4, sh, part + (g.m * gridDim.x + blockIdx.x) * 3, [&](double mu) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < kTnIter4; ++i)
      if (threadIdx.x + i * kTnThreads < g.n4) {
        const double d0 = (double)v[i].x - mu, d1 = (double)v[i].y - mu, d2 = (double)v[i].z - mu, d3 = (double)v[i].w - mu;
        q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
    return q;
  });
}

// ---- gLN -> float32 (the operand of the next product in the float32 validation mode) -------------------------------------------------
__global__ __launch_bounds__(kTnThreads) void gln_apply_f32_kernel(const float* __restrict__ y, int64_t K, int C, int rows,
                                                                   const double* __restrict__ part_in, int nparts_in,
                                                                   float* __restrict__ out) {
  __shared__ double sh[4];
  const TileGeom g = tile_geom(K, C, rows);
  float mean, rstd;
  gln_mean_rstd(part_in + g.m * nparts_in * 3, nparts_in, sh, mean, rstd);
#pragma unroll
  for (int i = 0; i < kTnIter4; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    if (e < g.n4) {
      float4 q = ld4(y + g.base + (int64_t)e * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) comp(q, j) = (comp(q, j) - mean) * rstd;
      *reinterpret_cast<float4*>(out + g.base + (int64_t)e * 4) = q;
    }
  }
}

// ---- d(-mean(max_snr)) / d estimate in closed form, float64 ----------------------------------------------------------------------------
// One workgroup per (b, target j); its estimate is i = perm[b, j].  With a = e - mean(e), r = t - mean(t) over the valid samples,
// dot = a . r, S = r . r, en = S + eps, proj = dot r / en, noise = a - proj, pp = |proj|^2 = dot^2 S / en^2, nn = |noise|^2,
// q = pp / (nn + eps), snr = 10 log10(q + eps):
//   d snr / d a = k [ (2 dot S / en^2) r / (nn + eps) - pp / (nn + eps)^2 (2 noise - 2 (noise . r / en) r) ],  k = 10 / (ln 10 (q + eps))
// and d / d e = d / d a minus its mean over the valid samples (a = e - sum(e) / len).  loss = -sum_{b, j} snr / (B C).
__global__ __launch_bounds__(kTnThreads) void si_snr_grad_kernel(const float* __restrict__ src, const float* __restrict__ est,
                                                                 const int64_t* __restrict__ lengths, const int64_t* __restrict__ perm,
                                                                 int64_t B, int C, int64_t T, float* __restrict__ grad) {
  __shared__ double sh[4];
  const int64_t id = blockIdx.x, b = id / C;
  const int j = (int)(id - b * C);
  int64_t i = perm[id];
  i = i < 0 ? 0 : i >= C ? C - 1 : i;  // (a permutation never leaves [0, C); a corrupt one must not leave the buffer)
  const int64_t len = lengths[b] < 0 ? 0 : lengths[b] > T ? T : lengths[b];
  const float* e = est + (b * C + i) * T;
  const float* t = src + (b * C + j) * T;
  float* o = grad + (b * C + i) * T;
  const double eps = 1e-8;
  double se = 0.0, st = 0.0;
  for (int64_t n = threadIdx.x; n < len; n += kTnThreads) {
    se += (double)e[n];
    st += (double)t[n];
  }
  const double num = (double)(len > 0 ? len : 1);
  const double me = tile_sum(se, sh) / num, mt = tile_sum(st, sh) / num;
  double dot = 0.0, S = 0.0;
  for (int64_t n = threadIdx.x; n < len; n += kTnThreads) {
    const double a = (double)e[n] - me, r = (double)t[n] - mt;
    dot += a * r;
    S += r * r;
  }
  dot = tile_sum(dot, sh);
  S = tile_sum(S, sh);
  const double en = S + eps;
  double pp = 0.0, nn = 0.0, nr = 0.0;
  for (int64_t n = threadIdx.x; n < len; n += kTnThreads) {
    const double a = (double)e[n] - me, r = (double)t[n] - mt;
    const double proj = dot * r / en, noise = a - proj;
    pp += proj * proj;
    nn += noise * noise;
    nr += noise * r;
  }
  pp = tile_sum(pp, sh);
  nn = tile_sum(nn, sh);
  nr = tile_sum(nr, sh);
  const double q = pp / (nn + eps);
  const double k = 10.0 / (log(10.0) * (q + eps)) * (-1.0 / ((double)B * (double)C));
  const double dpp = k / (nn + eps), dnn = -k * pp / ((nn + eps) * (nn + eps));
  const double cr = dpp * 2.0 * dot * S / (en * en) - dnn * 2.0 * nr / en, cn = dnn * 2.0;
  double gs = 0.0;
  for (int64_t n = threadIdx.x; n < len; n += kTnThreads) {
    const double a = (double)e[n] - me, r = (double)t[n] - mt;
    gs += cr * r + cn * (a - dot * r / en);
  }
  const double gm = tile_sum(gs, sh) / num;
  for (int64_t n = threadIdx.x; n < T; n += kTnThreads) {
    float v = 0.0f;
    if (n < len) {
      const double a = (double)e[n] - me, r = (double)t[n] - mt;
      v = (float)(cr * r + cn * (a - dot * r / en) - gm);
    }
    o[n] = v;
  }
}

// ---- the sum of outer products that the decoder's and the encoder's weight gradients are ---------------------------------------------
// out[l][n] += sum_item a[item][l] * b[item][n] over the kOpItems items staged in LDS; thread t owns the outputs t, t + 256, ...
// (at most kOpOut of them: L * N <= 256 kOpOut), output (l, n) at l * N + n.
constexpr int kOpItems = 16;
constexpr int kOpOut = 48;
constexpr int kOpChunks = 4;  // chunks of kOpItems items that one workgroup walks

__device__ __forceinline__ void outer_accumulate(const float* __restrict__ a, const float* __restrict__ b, int L, int N,
                                                 float (&acc)[kOpOut]) {
  const int total = L * N;
  int off_a[kOpOut], off_b[kOpOut];
#pragma unroll
  for (int j = 0; j < kOpOut; ++j) {
    const int o = threadIdx.x + j * kTnThreads;
    const int oo = o < total ? o : 0;
    off_a[j] = oo / N;
    off_b[j] = oo - off_a[j] * N;
  }
#pragma unroll 1
  for (int it = 0; it < kOpItems; ++it) {
#pragma unroll
    for (int j = 0; j < kOpOut; ++j)
      if (threadIdx.x + j * kTnThreads < total) acc[j] = fmaf(a[it * L + off_a[j]], b[it * N + off_b[j]], acc[j]);
  }
}

// ---- decoder + mask backward ------------------------------------------------------------------------------------------------------------
// d_out (M, C, (K + 1) hop) -> d_frame[l] = d_out[k hop + (paired ? l mod hop : l)];  d_source_w[n] = sum_l d_frame[l] basis[l, n];
// d_score = d_source_w * mixture_w * (score > 0);  d_mw[n] = sum_c d_source_w * relu(score);  d_basis[l, n] = sum d_frame[l] source_w[n].
// A chunk is kOpItems / C frames of one utterance, all sources; wave w takes the chunk's frames w, w + 4, ... and lane i the channels
// n = i, i + 64, ...; the workgroup walks kOpChunks chunks and leaves ONE d_basis partial.
__global__ __launch_bounds__(kTnThreads) void tasnet_decode_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ score,
                                                                       const float* __restrict__ mw, int64_t K, int C, int N,
                                                                       const float* __restrict__ basis, int L, int true_overlap,
                                                                       float* __restrict__ dscore, float* __restrict__ dmw,
                                                                       float* __restrict__ dbasis_part) {
  extern __shared__ __attribute__((aligned(16))) float op_lds[];
  float* sw = op_lds;                  // [kOpItems][N]
  float* df = op_lds + kOpItems * N;   // [kOpItems][L]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hop = L / 2, fpc = kOpItems / C;  // frames per chunk
  const int64_t m = blockIdx.y, nchunks = (K + fpc - 1) / fpc;
  float acc[kOpOut];
#pragma unroll
  for (int j = 0; j < kOpOut; ++j) acc[j] = 0.0f;
  for (int cw = 0; cw < kOpChunks; ++cw) {
    const int64_t chunk = (int64_t)blockIdx.x * kOpChunks + cw;
    if (chunk >= nchunks) break;  // (uniform over the workgroup)
    const int64_t k0 = chunk * fpc;
    for (int e = threadIdx.x; e < kOpItems * L; e += kTnThreads) {
      const int it = e / L, l = e - it * L, f = it / C, c = it - f * C;
      const int64_t k = k0 + f;
      float v = 0.0f;
      if (f < fpc && k < K) v = dout[(m * C + c) * ((K + 1) * hop) + k * hop + (true_overlap ? l : l % hop)];  // <= (K + 1) hop - 1
      df[e] = v;
    }
    __syncthreads();
    for (int f = wave; f * C < kOpItems; f += kTnThreads / 64) {
      const int64_t k = k0 + f;
      const bool live = f < fpc && k < K;
      for (int n = lane; n < N; n += 64) {
        float dm = 0.0f;
        for (int c = 0; c < C; ++c) {
          const int it = f * C + c;
          if (it >= kOpItems) break;
          float s = 0.0f;
          if (live) {
            float ds = 0.0f;
            for (int l = 0; l < L; ++l) ds = fmaf(df[it * L + l], basis[(int64_t)l * N + n], ds);
            const int64_t row = m * K + k;
            const float sc = score[row * ((int64_t)C * N) + (int64_t)c * N + n], w = mw[row * N + n];
            dscore[row * ((int64_t)C * N) + (int64_t)c * N + n] = sc > 0.0f ? ds * w : 0.0f;
            dm = fmaf(ds, fmaxf(sc, 0.0f), dm);
            s = fmaxf(sc, 0.0f) * w;
          }
          sw[it * N + n] = s;
        }
        if (live) dmw[(m * K + k) * N + n] = dm;
      }
    }
    __syncthreads();
    outer_accumulate(df, sw, L, N, acc);
    __syncthreads();
  }
  float* o = dbasis_part + (m * gridDim.x + blockIdx.x) * ((int64_t)L * N);
#pragma unroll
  for (int j = 0; j < kOpOut; ++j)
    if (threadIdx.x + j * kTnThreads < L * N) o[threadIdx.x + j * kTnThreads] = acc[j];
}

// ---- encoder backward --------------------------------------------------------------------------------------------------------------------
// d_mixture_w = (the decoder's share) + gLN backward of the bottleneck's input gradient d_nb;  g = d_mixture_w * (mixture_w > 0);
// d_Ut[l, n] = sum_{m, k} g[m, k, n] x[m, k hop + l].  A chunk is kOpItems frames; the partial is (L, N), the order of the forward's Wt.
__global__ __launch_bounds__(kTnThreads) void tasnet_encode_bwd_kernel(const float* __restrict__ x, int64_t ldx, int64_t K,
                                                                       const float* __restrict__ mw, const double* __restrict__ part_n,
                                                                       int nparts, const float* __restrict__ dnb,
                                                                       const double* __restrict__ part2, const float* __restrict__ dmw_dec,
                                                                       int L, int N, float* __restrict__ dU_part) {
  extern __shared__ __attribute__((aligned(16))) float op_lds[];
  __shared__ double sh[4];
  float* gs = op_lds;                  // [kOpItems][N]
  float* xf = op_lds + kOpItems * N;   // [kOpItems][L]
  const int hop = L / 2;
  const int64_t m = blockIdx.y, nchunks = (K + kOpItems - 1) / kOpItems;
  const GlnBwd st = gln_bwd_load(part_n + m * nparts * 3, part2 + m * nparts * 2, nparts, (double)K * (double)N, sh);
  const float mean = st.mean, rstd = st.rstd, m1 = st.m1, m2 = st.m2;
  float acc[kOpOut];
#pragma unroll
  for (int j = 0; j < kOpOut; ++j) acc[j] = 0.0f;
  for (int cw = 0; cw < kOpChunks; ++cw) {
    const int64_t chunk = (int64_t)blockIdx.x * kOpChunks + cw;
    if (chunk >= nchunks) break;
    const int64_t k0 = chunk * kOpItems;
    for (int e = threadIdx.x; e < kOpItems * L; e += kTnThreads) {
      const int it = e / L, l = e - it * L;
      const int64_t k = k0 + it;
      xf[e] = k < K ? x[m * ldx + k * hop + l] : 0.0f;  // k hop + l <= (K - 1) hop + L - 1 < T
    }
    for (int e = threadIdx.x; e < kOpItems * N; e += kTnThreads) {
      const int it = e / N, n = e - it * N;
      const int64_t k = k0 + it;
      float v = 0.0f;
      if (k < K) {
        const int64_t idx = (m * K + k) * N + n;
        const float w = mw[idx], xh = (w - mean) * rstd;
        const float d = dmw_dec[idx] + (dnb[idx] - m1 - xh * m2) * rstd;
        v = w > 0.0f ? d : 0.0f;
      }
      gs[e] = v;
    }
    __syncthreads();
    outer_accumulate(xf, gs, L, N, acc);
    __syncthreads();
  }
  float* o = dU_part + (m * gridDim.x + blockIdx.x) * ((int64_t)L * N);
#pragma unroll
  for (int j = 0; j < kOpOut; ++j)
    if (threadIdx.x + j * kTnThreads < L * N) o[threadIdx.x + j * kTnThreads] = acc[j];
}

// ---- (a) the two sums of a gLN backward: sum(dy), sum(dy * xhat), xhat from prelu(v, a) and the forward's moments ---------------------------
__global__ __launch_bounds__(kTnThreads) void gln_bwd_stats_kernel(const float* __restrict__ dy, const float* __restrict__ v, int64_t K,
                                                                   int C, int rows, const double* __restrict__ part_in, int nparts,
                                                                   const float* __restrict__ a_ptr, double* __restrict__ part2) {
  __shared__ double sh[4];
  const TileGeom g = tile_geom(K, C, rows);
  float mean, rstd;
  gln_mean_rstd(part_in + g.m * nparts * 3, nparts, sh, mean, rstd);
  const float a = a_ptr[0];
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int i = 0; i < kTnIter4; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    if (e < g.n4) {
      const float4 d = ld4(dy + g.base + (int64_t)e * 4), q = ld4(v + g.base + (int64_t)e * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xh = (prelu(comp(q, j), a) - mean) * rstd;
        s1 += (double)comp(d, j);
        s2 += (double)comp(d, j) * (double)xh;
      }
    }
  }
  s1 = tile_sum(s1, sh);
  s2 = tile_sum(s2, sh);
  if (threadIdx.x == 0) {
    double* o = part2 + (g.m * gridDim.x + blockIdx.x) * 2;
    o[0] = s1;
    o[1] = s2;
  }
}

// gLN backward + PReLU backward of ONE element: the gradient at the pre-activation `pre`, and (through dz) at the PReLU output
__device__ __forceinline__ float gln_prelu_bwd(float dy, float pre, float a, float mean, float rstd, float m1, float m2, float& dz) {
  const float xh = (prelu(pre, a) - mean) * rstd;
  dz = (dy - m1 - xh * m2) * rstd;
  return pre >= 0.0f ? dz : a * dz;
}

// ---- (b) gLN2 backward, PReLU2 backward, depthwise backward, and the sums of the gLN1 backward that follows --------------------------------
// d0[k] = w0 n1[k - d] + w1 n1[k] + w2 n1[k + d] (n1 = the normalised prelu(y0), 0 outside [0, K)), so
//   du[k] = w0 dd0[k + d] + w1 dd0[k] + w2 dd0[k - d]   (dd0 outside [0, K) does not exist: those taps are skipped)
//   dW[p, c] = sum_k dd0[k, c] n1[k + (p - 1) d, c]
// dd0 of the neighbouring rows is recomputed from dh and d0 there.  256 % (C / 4) == 0, so a thread keeps ONE group of four channels
// for all its rows and sums its tap gradients in registers; the threads of a channel group are then added in index order through LDS.
__global__ __launch_bounds__(kTnThreads) void gln2_bwd_dwconv_kernel(
    const float* __restrict__ dh, const float* __restrict__ d0, const float* __restrict__ y0, int64_t K, int C, int rows,
    const double* __restrict__ part_a, const double* __restrict__ part_b, int nparts, const double* __restrict__ part2_h,
    const float* __restrict__ a1_ptr, const float* __restrict__ a2_ptr, const float* __restrict__ Wt, int dil, float* __restrict__ du,
    double* __restrict__ part2_u, float* __restrict__ da2_part, float* __restrict__ dw_part) {
  __shared__ double sh[4];
  __shared__ float red[12][kTnThreads];
  const TileGeom g = tile_geom(K, C, rows);
  float mean1, rstd1;
  gln_mean_rstd(part_a + g.m * nparts * 3, nparts, sh, mean1, rstd1);
  const GlnBwd st = gln_bwd_load(part_b + g.m * nparts * 3, part2_h + g.m * nparts * 2, nparts, (double)K * (double)C, sh);
  const float mean2 = st.mean, rstd2 = st.rstd, m1 = st.m1, m2 = st.m2;
  const float a1 = a1_ptr[0], a2 = a2_ptr[0];
  const int64_t step = (int64_t)dil * C;
  const int c = (threadIdx.x % g.C4) * 4;  // the same for every i: kTnThreads % C4 == 0
  const float4 w0 = ld4(Wt + c), w1 = ld4(Wt + C + c), w2 = ld4(Wt + 2 * C + c);
  float4 gw[3];
  gw[0] = gw[1] = gw[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  double s1 = 0.0, s2 = 0.0, sa = 0.0;
#pragma unroll
  for (int i = 0; i < kTnIter4; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    if (e < g.n4) {
      const int r = e / g.C4;
      const int64_t k = g.row0 + r, at = g.base + (int64_t)e * 4;
      const bool lo = k - dil >= 0, hi = k + dil < K;
      const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float4 dh_c = ld4(dh + at), d0_c = ld4(d0 + at), y_c = ld4(y0 + at);
      const float4 dh_l = lo ? ld4(dh + at - step) : z4, d0_l = lo ? ld4(d0 + at - step) : z4, y_l = lo ? ld4(y0 + at - step) : z4;
      const float4 dh_h = hi ? ld4(dh + at + step) : z4, d0_h = hi ? ld4(d0 + at + step) : z4, y_h = hi ? ld4(y0 + at + step) : z4;
      float4 out;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float dz, dzn;
        const float dd_c = gln_prelu_bwd(comp(dh_c, j), comp(d0_c, j), a2, mean2, rstd2, m1, m2, dz);
        const float dd_l = lo ? gln_prelu_bwd(comp(dh_l, j), comp(d0_l, j), a2, mean2, rstd2, m1, m2, dzn) : 0.0f;
        const float dd_h = hi ? gln_prelu_bwd(comp(dh_h, j), comp(d0_h, j), a2, mean2, rstd2, m1, m2, dzn) : 0.0f;
        if (comp(d0_c, j) < 0.0f) sa += slope_term(comp(dh_c, j), comp(d0_c, j), a2, st);
        const float u = fmaf(comp(w0, j), dd_h, fmaf(comp(w1, j), dd_c, comp(w2, j) * dd_l));
        comp(out, j) = u;
        const float n_c = (prelu(comp(y_c, j), a1) - mean1) * rstd1;
        const float n_l = lo ? (prelu(comp(y_l, j), a1) - mean1) * rstd1 : 0.0f;
        const float n_h = hi ? (prelu(comp(y_h, j), a1) - mean1) * rstd1 : 0.0f;
        comp(gw[0], j) = fmaf(dd_c, n_l, comp(gw[0], j));
        comp(gw[1], j) = fmaf(dd_c, n_c, comp(gw[1], j));
        comp(gw[2], j) = fmaf(dd_c, n_h, comp(gw[2], j));
        s1 += (double)u;
        s2 += (double)u * (double)n_c;
      }
      *reinterpret_cast<float4*>(du + at) = out;
    }
  }
  s1 = tile_sum(s1, sh);
  s2 = tile_sum(s2, sh);
  sa = tile_sum(sa, sh);
  const int64_t tile = g.m * gridDim.x + blockIdx.x;
  if (threadIdx.x == 0) {
    part2_u[tile * 2] = s1;
    part2_u[tile * 2 + 1] = s2;
    da2_part[tile] = (float)sa;
  }
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[p * 4 + j][threadIdx.x] = comp(gw[p], j);
  __syncthreads();
  if ((int)threadIdx.x < g.C4) {
    float* o = dw_part + tile * (3 * (int64_t)C);  // (3, C): the order of Wt
    for (int q = 0; q < 12; ++q) {
      float s = 0.0f;
      for (int t = threadIdx.x; t < kTnThreads; t += g.C4) s += red[q][t];
      o[(q >> 2) * C + c + (q & 3)] = s;
    }
  }
}

// ---- (c) gLN1 backward, PReLU1 backward, the operand of the two products that follow ------------------------------------------------------
template <bool BF16>
__global__ __launch_bounds__(kTnThreads) void gln1_bwd_kernel(const float* __restrict__ du, const float* __restrict__ y0, int64_t K, int C,
                                                              int rows, const double* __restrict__ part_a, int nparts,
                                                              const double* __restrict__ part2_u, const float* __restrict__ a_ptr,
                                                              void* __restrict__ out, float* __restrict__ da_part) {
  __shared__ double sh[4];
  const TileGeom g = tile_geom(K, C, rows);
  const GlnBwd st = gln_bwd_load(part_a + g.m * nparts * 3, part2_u + g.m * nparts * 2, nparts, (double)K * (double)C, sh);
  const float mean = st.mean, rstd = st.rstd, m1 = st.m1, m2 = st.m2;
  const float a = a_ptr[0];
  double sa = 0.0;
#pragma unroll
  for (int i = 0; i < kTnIter4; ++i) {
    const int e = threadIdx.x + i * kTnThreads;
    if (e < g.n4) {
      const int64_t at = g.base + (int64_t)e * 4;
      const float4 d = ld4(du + at), q = ld4(y0 + at);
      float4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float dz;
        comp(r, j) = gln_prelu_bwd(comp(d, j), comp(q, j), a, mean, rstd, m1, m2, dz);
        if (comp(q, j) < 0.0f) sa += slope_term(comp(d, j), comp(q, j), a, st);
      }
      if (BF16) {
        uint2 o;
        o.x = (uint32_t)f2bf(r.x) | ((uint32_t)f2bf(r.y) << 16);
        o.y = (uint32_t)f2bf(r.z) | ((uint32_t)f2bf(r.w) << 16);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out) + at) = o;
      } else {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + at) = r;
      }
    }
  }
  sa = tile_sum(sa, sh);
  if (threadIdx.x == 0) da_part[g.m * gridDim.x + blockIdx.x] = (float)sa;
}

// ---- nn.SGD(momentum, weight_decay) + the bf16 mirror of the updated parameters ----------------------------------------------------------
__global__ __launch_bounds__(256) void sgd_momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                           int64_t n4, float lr, float momentum, float wd, int first,
                                                           uint16_t* __restrict__ mirror) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 pv = ld4(p + i * 4);
    const float4 gv = ld4(g + i * 4);
    float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (momentum > 0.0f && !first) bv = ld4(buf + i * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float d = fmaf(wd, comp(pv, j), comp(gv, j));
      if (momentum > 0.0f) {
        d = first ? d : fmaf(momentum, comp(bv, j), d);
        comp(bv, j) = d;
      }
      comp(pv, j) = comp(pv, j) - lr * d;
    }
    *reinterpret_cast<float4*>(p + i * 4) = pv;
    if (momentum > 0.0f) *reinterpret_cast<float4*>(buf + i * 4) = bv;
    if (mirror) {
      uint2 o;
      o.x = (uint32_t)f2bf(pv.x) | ((uint32_t)f2bf(pv.y) << 16);
      o.y = (uint32_t)f2bf(pv.z) | ((uint32_t)f2bf(pv.w) << 16);
      *reinterpret_cast<uint2*>(mirror + i * 4) = o;
    }
  }
}

// shape checks of the launches (b) and (c) and their forward: check_tiles + one channel group per thread
static int check_train_tiles(int64_t M, int64_t K, int32_t C, int64_t* tiles) {
  const int rc = check_tiles(M, K, C, tiles);
  if (rc != MA_OK) return rc;
  if (kTnThreads % (C / 4) != 0) return MA_ERR_UNSUPPORTED;  // C in {64, 128, 256, 512, 1024}
  return MA_OK;
}

static int check_outer(int64_t M, int64_t K, int32_t L, int32_t N, int32_t items_per_frame, int64_t* groups, size_t* lds) {
  if (M < 1 || K < 1 || L < 2 || N < 1 || items_per_frame < 1) return MA_ERR_INVALID_ARG;
  *lds = (size_t)kOpItems * (size_t)(N + L) * sizeof(float);
  if ((L & 1) || L > 64 || N % 64 != 0 || (int64_t)L * N > (int64_t)kOpOut * kTnThreads || *lds > 60 * 1024 ||
      items_per_frame > kOpItems || M > 65535 || M * K > 0x7fffffff)
    return MA_ERR_UNSUPPORTED;
  const int64_t fpc = kOpItems / items_per_frame, chunks = (K + fpc - 1) / fpc;
  *groups = (chunks + kOpChunks - 1) / kOpChunks;
  return MA_OK;
}

}  // namespace ma

using namespace ma;

extern "C" int ma_gln_dwconv_prelu_train(const float* y, int64_t M, int64_t K, int32_t C, const double* part_in, const float* Wt,
                                         int32_t P, int32_t dilation, const float* weight, float* pre, float* z, double* part_out,
                                         ma_stream_t stream) {
  if (!y || !part_in || !Wt || !weight || !pre || !z || !part_out || P < 1 || dilation < 1 || z == y || pre == y || pre == z)
    return MA_ERR_INVALID_ARG;
  if (P != 3) return MA_ERR_UNSUPPORTED;
  int64_t tiles = 0;
  const int rc = check_tiles(M, K, C, &tiles);
  if (rc != MA_OK) return rc;
  if (!aligned16(y) || !aligned16(z) || !aligned16(pre) || !aligned16(Wt)) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(gln_dwconv_prelu_train_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, y, K, C,
            tile_rows(C), part_in, (int)tiles, Wt, dilation, weight, pre, z, part_out);
  return MA_OK;
}

extern "C" int ma_gln_apply_f32(const float* y, int64_t M, int64_t K, int32_t C, const double* part, float* out, ma_stream_t stream) {
  if (!y || !part || !out) return MA_ERR_INVALID_ARG;
  int64_t tiles = 0;
  const int rc = check_tiles(M, K, C, &tiles);
  if (rc != MA_OK) return rc;
  if (!aligned16(y) || !aligned16(out)) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(gln_apply_f32_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, y, K, C, tile_rows(C), part,
            (int)tiles, out);
  return MA_OK;
}

extern "C" int ma_si_snr_grad_f32(const float* source, const float* estimate, const int64_t* lengths, const int64_t* perm, int64_t B,
                                  int32_t C, int64_t T, float* grad, ma_stream_t stream) {
  if (!source || !estimate || !lengths || !perm || !grad || B < 1 || C < 1 || T < 1) return MA_ERR_INVALID_ARG;
  if (C > 8 || B * C > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(si_snr_grad_kernel, dim3((unsigned)(B * C)), dim3(kTnThreads), 0, (hipStream_t)stream, source, estimate, lengths, perm, B, C,
            T, grad);
  return MA_OK;
}

extern "C" int32_t ma_tasnet_decode_bwd_parts(int64_t K, int32_t C, int32_t N, int32_t L) {
  int64_t groups = 0;
  size_t lds = 0;
  if (C < 1 || check_outer(1, K, L, N, C, &groups, &lds) != MA_OK || groups > 0x7fffffff) return 0;
  return (int32_t)groups;
}

extern "C" int ma_tasnet_decode_bwd_f32(const float* d_out, const float* score, const float* mixture_w, int64_t M, int64_t K, int32_t C,
                                        int32_t N, const float* basis, int32_t L, int32_t overlap, float* d_score, float* d_mixture_w,
                                        float* d_basis_part, ma_stream_t stream) {
  if (!d_out || !score || !mixture_w || !basis || !d_score || !d_mixture_w || !d_basis_part || C < 1) return MA_ERR_INVALID_ARG;
  if (overlap != MA_TASNET_OVERLAP_PAIRED && overlap != MA_TASNET_OVERLAP_TRUE) return MA_ERR_INVALID_ARG;
  int64_t groups = 0;
  size_t lds = 0;
  const int rc = check_outer(M, K, L, N, C, &groups, &lds);
  if (rc != MA_OK) return rc;
  if (groups > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(tasnet_decode_bwd_kernel, dim3((unsigned)groups, (unsigned)M), dim3(kTnThreads), lds, (hipStream_t)stream, d_out, score,
            mixture_w, K, C, N, basis, L, overlap == MA_TASNET_OVERLAP_TRUE ? 1 : 0, d_score, d_mixture_w, d_basis_part);
  return MA_OK;
}

extern "C" int32_t ma_tasnet_encode_bwd_parts(int64_t K, int32_t N, int32_t L) {
  int64_t groups = 0;
  size_t lds = 0;
  if (check_outer(1, K, L, N, 1, &groups, &lds) != MA_OK || groups > 0x7fffffff) return 0;
  return (int32_t)groups;
}

extern "C" int ma_tasnet_encode_bwd_f32(const float* x, int64_t M, int64_t T, int64_t ldx, const float* mixture_w, const double* part,
                                        const float* d_norm, const double* part2, const float* d_mixture_w, int32_t L, int32_t N,
                                        float* d_Ut_part, ma_stream_t stream) {
  if (!x || !mixture_w || !part || !d_norm || !part2 || !d_mixture_w || !d_Ut_part || L < 2 || T < L || ldx < T) return MA_ERR_INVALID_ARG;
  if (L & 1) return MA_ERR_UNSUPPORTED;
  const int64_t K = (T - L) / (L / 2) + 1;
  int64_t groups = 0, tiles = 0;
  size_t lds = 0;
  int rc = check_outer(M, K, L, N, 1, &groups, &lds);
  if (rc != MA_OK) return rc;
  rc = check_tiles(M, K, N, &tiles);
  if (rc != MA_OK) return rc;
  if (groups > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(tasnet_encode_bwd_kernel, dim3((unsigned)groups, (unsigned)M), dim3(kTnThreads), lds, (hipStream_t)stream, x, ldx, K, mixture_w,
            part, (int)tiles, d_norm, part2, d_mixture_w, L, N, d_Ut_part);
  return MA_OK;
}

extern "C" int ma_gln_bwd_stats(const float* dy, const float* v, int64_t M, int64_t K, int32_t C, const double* part, const float* weight,
                                double* part2, ma_stream_t stream) {
  if (!dy || !v || !part || !weight || !part2) return MA_ERR_INVALID_ARG;
  int64_t tiles = 0;
  const int rc = check_tiles(M, K, C, &tiles);
  if (rc != MA_OK) return rc;
  if (!aligned16(dy) || !aligned16(v)) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(gln_bwd_stats_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, dy, v, K, C, tile_rows(C),
            part, (int)tiles, weight, part2);
  return MA_OK;
}

extern "C" int ma_gln2_bwd_dwconv(const float* d_h, const float* d0, const float* y0, int64_t M, int64_t K, int32_t C, const double* part_a,
                                  const double* part_b, const double* part2_h, const float* weight1, const float* weight2,
                                  const float* Wt, int32_t P, int32_t dilation, float* d_u, double* part2_u, float* d_weight2_part,
                                  float* d_Wt_part, ma_stream_t stream) {
  if (!d_h || !d0 || !y0 || !part_a || !part_b || !part2_h || !weight1 || !weight2 || !Wt || !d_u || !part2_u || !d_weight2_part ||
      !d_Wt_part || P < 1 || dilation < 1 || d_u == d_h || d_u == d0 || d_u == y0)
    return MA_ERR_INVALID_ARG;
  if (P != 3) return MA_ERR_UNSUPPORTED;
  int64_t tiles = 0;
  const int rc = check_train_tiles(M, K, C, &tiles);
  if (rc != MA_OK) return rc;
  if (!aligned16(d_h) || !aligned16(d0) || !aligned16(y0) || !aligned16(d_u) || !aligned16(Wt)) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(gln2_bwd_dwconv_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, d_h, d0, y0, K, C,
            tile_rows(C), part_a, part_b, (int)tiles, part2_h, weight1, weight2, Wt, dilation, d_u, part2_u, d_weight2_part, d_Wt_part);
  return MA_OK;
}

extern "C" int ma_gln1_bwd(const float* d_u, const float* y0, int64_t M, int64_t K, int32_t C, const double* part_a, const double* part2_u,
                           const float* weight, void* out, int32_t out_bf16, float* d_weight_part, ma_stream_t stream) {
  if (!d_u || !y0 || !part_a || !part2_u || !weight || !out || !d_weight_part) return MA_ERR_INVALID_ARG;
  int64_t tiles = 0;
  const int rc = check_tiles(M, K, C, &tiles);
  if (rc != MA_OK) return rc;
  if (!aligned16(d_u) || !aligned16(y0) || !aligned16(out)) return MA_ERR_INVALID_ARG;
  if (out_bf16)
    MA_LAUNCH(gln1_bwd_kernel<true>, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, d_u, y0, K, C,
              tile_rows(C), part_a, (int)tiles, part2_u, weight, out, d_weight_part);
  else
    MA_LAUNCH(gln1_bwd_kernel<false>, dim3((unsigned)tiles, (unsigned)M), dim3(kTnThreads), 0, (hipStream_t)stream, d_u, y0, K, C,
              tile_rows(C), part_a, (int)tiles, part2_u, weight, out, d_weight_part);
  return MA_OK;
}

extern "C" int ma_sgd_momentum_f32(float* param, const float* grad, float* buf, int64_t n, float lr, float momentum, float weight_decay,
                                   int32_t first_step, void* mirror_bf16, ma_stream_t stream) {
  if (!param || !grad || n < 1 || momentum < 0.0f || (momentum > 0.0f && !buf)) return MA_ERR_INVALID_ARG;
  if ((n & 3) || !aligned16(param) || !aligned16(grad) || (buf && !aligned16(buf)) || (reinterpret_cast<uintptr_t>(mirror_bf16) & 7))
    return MA_ERR_UNSUPPORTED;
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  MA_LAUNCH(sgd_momentum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, buf, n / 4, lr, momentum,
            weight_decay, first_step ? 1 : 0, reinterpret_cast<uint16_t*>(mirror_bf16));
  return MA_OK;
}
