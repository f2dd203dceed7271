// ECAPA speaker-classification head on gfx950: everything behind the embedding, forward and backward.
// (mindaudio/models/ecapatdnn.py: Classifier.construct 477-488 with lin_blocks = 0; mindaudio/loss/AdditiveAngularMargin.py;
//  SoftmaxCrossEntropyWithLogits(sparse=False, reduction="mean") and CorrectLabelNum of examples/ECAPA-TDNN/train_speaker_embeddings.py)
//
//   ma_aam_softmax_fwd_f32   3 launches: inverse norms of the rows of x and W -> cosine GEMM with the margin, the scaled output and
//                            per-(row, 32-class block) softmax partials in its epilogue -> one workgroup that joins the partials in
//                            block order into the log-sum-exp, the row losses, their mean and the number of correct rows
//   ma_aam_softmax_bwd_f32   3 launches: dW' = G^T e (one workgroup per 32 classes) -> de partials = G w over slabs of classes (one
//                            workgroup per 32 rows and slab) -> per row of x and W: the slabs summed in slab order, the Jacobian of the
//                            normalisation, l2 * W.  G = d loss / d cosine is recomputed from the stored output and log-sum-exp.
//   ma_aam_cosine_f32        Classifier.construct alone (the first two launches of the forward, no labels)
//   ma_aam_margin_f32        AdditiveAngularMargin.construct on given cosines and one-hot targets (elementwise)
//
// float32 throughout: v_mfma_f32_32x32x2_f32 on float32 operands (exact products, float32 accumulation), accurate expf / logf; the
// few per-row sums (squared norms, softmax denominators, the slab sums) are carried in float64 and rounded once.  No floating-point
// atomics: every sum that crosses waves or workgroups goes through a buffer and is added in index order, so two runs give the same
// bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "device_common.h"
#include "launch.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct Margin {
  float cos_m, sin_m, th, mm;
  int easy;
};

// phi of AdditiveAngularMargin.construct; sqrt(max(., 0)): rounding can push |c| past 1, where the reference yields NaN
__device__ __forceinline__ float margin_phi(float c, const Margin& p) {
  const float sine = sqrtf(fmaxf(1.f - c * c, 0.f));
  const float phi = c * p.cos_m - sine * p.sin_m;
  if (p.easy) return c > 0.f ? phi : c;
  return c > p.th ? phi : c - p.mm;
}
// d phi / d c; the floor on the sine keeps it finite at |c| = 1
__device__ __forceinline__ float margin_dphi(float c, const Margin& p) {
  const bool on = p.easy ? c > 0.f : c > p.th;
  if (!on) return 1.f;
  const float sine = sqrtf(fmaxf(1.f - c * c, 0.f));
  return p.cos_m + p.sin_m * c / fmaxf(sine, 0x1p-12f);
}

// sum of squares of one row, one wave per row: the forward's norm and the backward's saturation test use the same bits
__device__ __forceinline__ double row_sumsq(const float* __restrict__ row, int D, int lane) {
  double s = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)row[d];
    s += v * v;
  }
  return ma::wave_sum(s);
}

// inv[r] = 1 / sqrt(max(sum x[r]^2, eps)) for the rows of x (B) then W (N): MindSpore's L2Normalize
__global__ __launch_bounds__(256) void aam_norms_kernel(const float* __restrict__ x, int64_t B, const float* __restrict__ W, int64_t N,
                                                        int D, float eps, float* __restrict__ invx, float* __restrict__ invw) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B + N) return;
  const int lane = threadIdx.x & 63;
  const bool isx = r < B;
  const int64_t row = isx ? r : r - B;
  const double ss = row_sumsq((isx ? x : W) + row * D, D, lane);
  if (lane == 0) (isx ? invx : invw)[row] = (float)(1.0 / sqrt(fmax(ss, (double)eps)));
}

constexpr int FT = 64;   // rows and classes per forward tile (2 x 2 waves of one 32 x 32 block each)
constexpr int TK = 32;   // k per LDS chunk
constexpr int LDF = 96;  // LDS row stride: lanes 32..63 read k + 1, 96 % 64 = 32 puts them on the other 32 banks

// out[b][n] = s * (n == y[b] ? phi(c) : c), c = (x[b] invx[b]) . (W[n] invw[n]).  grid (ceil(N / 64), ceil(B / 64)).
// y == nullptr: no row has a target (the plain cosines with s = 1); pmax == nullptr: no softmax partials.
// pmax / psum / parg [b * nblk + blk]: maximum, sum of exp(out - maximum) and first arg-maximum over the valid classes of block blk.
__global__ __launch_bounds__(256) void aam_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                      const int32_t* __restrict__ y, const float* __restrict__ invx,
                                                      const float* __restrict__ invw, int64_t B, int64_t N, int D, float s, Margin mg,
                                                      float* __restrict__ out, float* __restrict__ pmax, float* __restrict__ psum,
                                                      int32_t* __restrict__ parg, float* __restrict__ tout, float* __restrict__ tgrad,
                                                      int64_t nblk) {
  __shared__ float As[TK * LDF];
  __shared__ float Bs[TK * LDF];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t n0 = (int64_t)blockIdx.x * FT;
  const int64_t m0 = (int64_t)blockIdx.y * FT;
  const int lr = tid & 63, lq = tid >> 6;  // loader: row of the tile, float4 slots lq and lq + 4 of the chunk's 8
  // rows past the end are read from the tile's first row (always inside); they only feed outputs that are never stored
  const int64_t ar = m0 + lr < B ? m0 + lr : m0;
  const int64_t br = n0 + lr < N ? n0 + lr : n0;
  const float* ap = x + ar * D;
  const float* bp = W + br * D;
  const float sa = invx[ar], sb = invw[br];

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  float4 pa[2], pb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    pa[j] = *reinterpret_cast<const float4*>(ap + 4 * (lq + 4 * j));
    pb[j] = *reinterpret_cast<const float4*>(bp + 4 * (lq + 4 * j));
  }
  const int chunks = D / TK;
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = 4 * (lq + 4 * j);
      As[(k + 0) * LDF + lr] = pa[j].x * sa;
      As[(k + 1) * LDF + lr] = pa[j].y * sa;
      As[(k + 2) * LDF + lr] = pa[j].z * sa;
      As[(k + 3) * LDF + lr] = pa[j].w * sa;
      Bs[(k + 0) * LDF + lr] = pb[j].x * sb;
      Bs[(k + 1) * LDF + lr] = pb[j].y * sb;
      Bs[(k + 2) * LDF + lr] = pb[j].z * sb;
      Bs[(k + 3) * LDF + lr] = pb[j].w * sb;
    }
    __syncthreads();
    if (c + 1 < chunks) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        pa[j] = *reinterpret_cast<const float4*>(ap + (c + 1) * TK + 4 * (lq + 4 * j));
        pb[j] = *reinterpret_cast<const float4*>(bp + (c + 1) * TK + 4 * (lq + 4 * j));
      }
    }
    const float* a_l = As + (lane >> 5) * LDF + wm * 32 + (lane & 31);
    const float* b_l = Bs + (lane >> 5) * LDF + wn * 32 + (lane & 31);
    // one fmaf chain per 32-deep chunk, added to the total once: chains of 32 + D / 32 instead of one of D
    f32x16 part;
#pragma unroll
    for (int r = 0; r < 16; ++r) part[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < TK / 2; ++kk)
      part = __builtin_amdgcn_mfma_f32_32x32x2f32(a_l[2 * kk * LDF], b_l[2 * kk * LDF], part, 0, 0, 0);
    acc += part;
  }

  // C/D map of the 32x32 forms: column = lane & 31 (class), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (batch row)
  const int64_t nb0 = n0 + wn * 32;
  if (nb0 >= N) return;  // (wave-uniform) the whole block lies past the last class
  const int64_t blk = nb0 >> 5;
  const int64_t n = nb0 + (lane & 31);
  const bool vn = n < N;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t b = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const bool vb = b < B;
    const float c = acc[r];
    const bool tgt = vb && vn && y != nullptr && (int64_t)y[b] == n;
    const float o = s * (tgt ? margin_phi(c, mg) : c);
    if (vb && vn) out[b * N + n] = o;
    if (tgt && tout != nullptr) {
      tout[b] = o;
      tgrad[b] = margin_dphi(c, mg);
    }
    if (pmax == nullptr) continue;
    float v = vn ? o : -INFINITY;
    int32_t idx = (int32_t)(vn ? n : 0x7fffffff);
#pragma unroll
    for (int sh = 16; sh > 0; sh >>= 1) {  // stays inside each half of the wave: 32 classes of one batch row
      const float ov = __shfl_xor(v, sh, 64);
      const int32_t oi = __shfl_xor(idx, sh, 64);
      if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
      }
    }
    float e = vn ? expf(o - v) : 0.f;
#pragma unroll
    for (int sh = 16; sh > 0; sh >>= 1) e += __shfl_xor(e, sh, 64);
    if ((lane & 31) == 0 && vb) {
      pmax[b * nblk + blk] = v;
      psum[b * nblk + blk] = e;
      parg[b * nblk + blk] = idx;
    }
  }
}

constexpr int FIN_THREADS = 1024;

// One workgroup: per batch row the blocks joined in block order (lse, row loss, arg-maximum), then the mean loss and the number of
// correct rows, each wave's rows in row order and the waves in wave order.  A row whose label lies outside [0, N) has no target.
__global__ __launch_bounds__(FIN_THREADS) void aam_fwd_finish_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                                     const int32_t* __restrict__ parg, const float* __restrict__ tout,
                                                                     const int32_t* __restrict__ y, int64_t B, int64_t N, int64_t nblk,
                                                                     float* __restrict__ lse, float* __restrict__ row_loss,
                                                                     float* __restrict__ loss, int32_t* __restrict__ correct) {
  __shared__ double wsum[FIN_THREADS / 64];
  __shared__ int32_t wcnt[FIN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double sum = 0.0;
  int32_t cnt = 0;
  for (int64_t b = wave; b < B; b += FIN_THREADS / 64) {
    const float* pm = pmax + b * nblk;
    float v = -INFINITY;
    int32_t idx = 0x7fffffff;
    for (int64_t k = lane; k < nblk; k += 64) {  // increasing class index: a strict comparison keeps the first maximum
      const float ov = pm[k];
      if (ov > v) {
        v = ov;
        idx = parg[b * nblk + k];
      }
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
      const float ov = __shfl_xor(v, sh, 64);
      const int32_t oi = __shfl_xor(idx, sh, 64);
      if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
      }
    }
    double se = 0.0;
    for (int64_t k = lane; k < nblk; k += 64) se += (double)psum[b * nblk + k] * (double)expf(pm[k] - v);
    se = ma::wave_sum(se);
    const float l = (float)((double)v + log(se));
    const int64_t yb = y[b];
    const bool has = yb >= 0 && yb < N;
    const float rl = has ? l - tout[b] : l;
    if (lane == 0) {
      lse[b] = l;
      row_loss[b] = rl;
    }
    sum += (double)rl;
    cnt += (has && (int64_t)idx == yb) ? 1 : 0;
  }
  if (lane == 0) {
    wsum[wave] = sum;
    wcnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    int32_t c = 0;
    for (int w = 0; w < FIN_THREADS / 64; ++w) {
      a += wsum[w];
      c += wcnt[w];
    }
    loss[0] = (float)(a / (double)B);
    correct[0] = c;
  }
}

constexpr int BM = 32;        // result rows per workgroup (one MFMA row block); the 4 waves share the D / 32 column blocks
constexpr int BK = 16;        // k per LDS chunk
constexpr int LDB_MAX = 544;  // D + 32 when D % 64 == 0, else D: the stride is 32 mod 64 either way

// d loss / d cosine[b][n], recomputed: coef (softmax - onehot), the target column times d phi / d c
__device__ __forceinline__ float g_elem(const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ tgrad,
                                        const int32_t* __restrict__ y, int64_t b, int64_t n, int64_t N, float coef) {
  const float p = expf(out[b * N + n] - lse[b]);
  if ((int64_t)y[b] == n) return coef * (p - 1.f) * tgrad[b];
  return coef * p;
}

// dst[m][d] = sum_k G(k, m) src[k][d] inv[k]
//   DX = false: m = class, k = batch row in [0, B): dW' = G^T e, dst (N, D).                      grid (ceil(N / 32), 1)
//   DX = true:  m = batch row, k = class in slab blockIdx.y: de partial = G w, dst (S, B, D).     grid (ceil(B / 32), S)
template <bool DX>
__global__ __launch_bounds__(256) void aam_bwd_gemm_kernel(const float* __restrict__ out, const float* __restrict__ lse,
                                                           const float* __restrict__ tgrad, const int32_t* __restrict__ y,
                                                           const float* __restrict__ src, const float* __restrict__ inv,
                                                           const float* __restrict__ grad_scale, float s, int64_t B, int64_t N, int D,
                                                           int64_t slab, float* __restrict__ dst) {
  __shared__ float As[BK * BM];
  __shared__ float Bs[BK * LDB_MAX];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ldb = (D % 64 == 0) ? D + 32 : D;
  const int d4 = D >> 2;
  const int ncb = D >> 5;
  const int64_t M = DX ? B : N;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int64_t k0 = DX ? (int64_t)blockIdx.y * slab : 0;
  const int64_t k1 = DX ? (k0 + slab < N ? k0 + slab : N) : B;
  const float coef = grad_scale[0] * s / (float)B;

  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // loader of G: 16 x 32 values per chunk, two per thread, along the contiguous axis of `out` (classes)
  const int am = DX ? (tid >> 4) : (tid & 31);  // second value: am + 16 (DX) / ak + 8
  const int ak = DX ? (tid & 15) : (tid >> 5);

  for (int64_t kb = k0; kb < k1; kb += BK) {
    float ga[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t m = m0 + am + (DX ? 16 * j : 0);
      const int64_t k = kb + ak + (DX ? 0 : 8 * j);
      const bool ok = m < M && k < k1;
      ga[j] = ok ? (DX ? g_elem(out, lse, tgrad, y, m, k, N, coef) : g_elem(out, lse, tgrad, y, k, m, N, coef)) : 0.f;
    }
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int j = 0; j < 2; ++j) As[(ak + (DX ? 0 : 8 * j)) * BM + am + (DX ? 16 * j : 0)] = ga[j];
    for (int i = tid; i < BK * d4; i += 256) {
      const int kr = i / d4, c4 = i - kr * d4;
      const bool ok = kb + kr < k1;
      const int64_t row = ok ? kb + kr : k0;  // rows past the range are read inside it and scaled by zero
      const float4 v = *reinterpret_cast<const float4*>(src + row * D + 4 * c4);
      const float sc = ok ? inv[row] : 0.f;
      float* q = Bs + kr * ldb + 4 * c4;
      q[0] = v.x * sc;
      q[1] = v.y * sc;
      q[2] = v.z * sc;
      q[3] = v.w * sc;
    }
    __syncthreads();
    const float* a_l = As + (lane >> 5) * BM + (lane & 31);
    const float* b_l = Bs + (lane >> 5) * ldb + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const float a = a_l[2 * kk * BM];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cb = wave + 4 * i;
        if (cb < ncb) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b_l[2 * kk * ldb + cb * 32], acc[i], 0, 0, 0);
      }
    }
  }
  float* o = dst + (DX ? (int64_t)blockIdx.y * B * D : 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cb = wave + 4 * i;
    if (cb >= ncb) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m < M) o[m * D + cb * 32 + (lane & 31)] = acc[i][r];
    }
  }
}

// One wave per row of x (B) then W (N).  v = d loss / d (normalised row): the slab partials added in slab order (x), or what the
// class GEMM left in dW (W, rewritten in place).  Through the normalisation u = r inv: inv (v - u (u . v)), or inv v where
// sum r^2 <= eps made the normalisation a division by the constant sqrt(eps).  W rows also receive l2 * W.
__global__ __launch_bounds__(256) void aam_bwd_finish_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                             const float* __restrict__ invx, const float* __restrict__ invw,
                                                             int64_t B, int64_t N, int D, float eps, float l2,
                                                             const float* __restrict__ part, int64_t S, float* __restrict__ dx,
                                                             float* __restrict__ dW) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B + N) return;
  const int lane = threadIdx.x & 63;
  const bool isx = r < B;
  const int64_t row = isx ? r : r - B;
  const float* src = (isx ? x : W) + row * D;
  float* dst = (isx ? dx : dW) + row * D;
  const float inv = (isx ? invx : invw)[row];
  const bool sat = row_sumsq(src, D, lane) <= (double)eps;
  float v[8], u[8], raw[8];
  double dot = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = lane + 64 * j;
    v[j] = u[j] = raw[j] = 0.f;
    if (d < D) {
      if (isx) {
        double a = 0.0;
        for (int64_t sl = 0; sl < S; ++sl) a += (double)part[(sl * B + row) * D + d];
        v[j] = (float)a;
      } else {
        v[j] = dst[d];
      }
      raw[j] = src[d];
      u[j] = raw[j] * inv;
      dot += (double)u[j] * (double)v[j];
    }
  }
  dot = ma::wave_sum(dot);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = lane + 64 * j;
    if (d < D) {
      const double t = sat ? (double)v[j] : (double)v[j] - (double)u[j] * dot;
      float g = (float)((double)inv * t);
      if (!isx) g = fmaf(l2, raw[j], g);
      dst[d] = g;
    }
  }
}

__global__ __launch_bounds__(256) void aam_margin_kernel(const float* __restrict__ cosine, const float* __restrict__ targets, int64_t n,
                                                         float s, Margin mg, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float c = cosine[i], t = targets[i];
  out[i] = s * (t * margin_phi(c, mg) + (1.f - t) * c);
}

bool width_ok(int32_t D) { return D >= 32 && D <= 512 && D % 32 == 0; }
bool shape_ok(int64_t B, int64_t N) { return B >= 1 && N >= 2 && N <= 0x7fffffff && B <= (int64_t)65535 * FT; }
int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

Margin make_margin(float margin, int32_t easy) {
  const double m = (double)margin, pi = 3.14159265358979323846;
  Margin mg;
  mg.cos_m = (float)cos(m);
  mg.sin_m = (float)sin(m);
  mg.th = (float)cos(pi - m);
  mg.mm = (float)(sin(pi - m) * m);
  mg.easy = easy ? 1 : 0;
  return mg;
}

// slabs of classes for the de partials: enough workgroups to fill the device, at most 64 slabs, each a multiple of the k chunk
void slabs_of(int64_t B, int64_t N, int64_t* slab, int64_t* S) {
  const int64_t row_tiles = (B + BM - 1) / BM;
  int64_t want = (384 + row_tiles - 1) / row_tiles;
  if (want > 64) want = 64;
  if (want < 1) want = 1;
  int64_t sl = round_up((N + want - 1) / want, BK);
  *slab = sl;
  *S = (N + sl - 1) / sl;
}

int64_t fwd_bytes(int64_t B, int64_t N) {
  const int64_t nblk = (N + 31) / 32;
  return 3 * round_up(B * nblk * 4, 256) + round_up(B * 4, 256);
}
int64_t bwd_bytes(int64_t B, int64_t D, int64_t N) {
  int64_t slab, S;
  slabs_of(B, N, &slab, &S);
  return round_up(S * B * D * 4, 256);
}

}  // namespace

extern "C" {

int64_t ma_aam_softmax_workspace_bytes(int64_t B, int32_t D, int64_t N) {
  if (!shape_ok(B, N)) return MA_ERR_INVALID_ARG;
  if (!width_ok(D)) return MA_ERR_UNSUPPORTED;
  const int64_t f = fwd_bytes(B, N), b = bwd_bytes(B, D, N);
  return f > b ? f : b;
}

int ma_aam_cosine_f32(const float* x, const float* W, int64_t B, int32_t D, int64_t N, float eps, float* cosine, float* inv_x,
                      float* inv_w, ma_stream_t stream) {
  if (!x || !W || !cosine || !inv_x || !inv_w || !shape_ok(B, N) || !(eps > 0.f)) return MA_ERR_INVALID_ARG;
  if (!width_ok(D)) return MA_ERR_UNSUPPORTED;
  if (((uintptr_t)x & 15) || ((uintptr_t)W & 15)) return MA_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MA_LAUNCH(aam_norms_kernel, dim3((unsigned)((B + N + 3) / 4)), dim3(256), 0, st, x, B, W, N, (int)D, eps, inv_x, inv_w);
  const Margin mg = make_margin(0.f, 0);
  MA_LAUNCH(aam_fwd_kernel, dim3((unsigned)((N + FT - 1) / FT), (unsigned)((B + FT - 1) / FT)), dim3(256), 0, st, x, W,
            (const int32_t*)nullptr, (const float*)inv_x, (const float*)inv_w, B, N, (int)D, 1.f, mg, cosine, (float*)nullptr,
            (float*)nullptr, (int32_t*)nullptr, (float*)nullptr, (float*)nullptr, (int64_t)0);
  return MA_OK;
}

int ma_aam_softmax_fwd_f32(const float* x, const float* W, const int32_t* y, int64_t B, int32_t D, int64_t N, float margin, float scale,
                           int32_t easy_margin, float eps, float* output, float* row_loss, float* loss, int32_t* correct, float* inv_x,
                           float* inv_w, float* lse, float* tgrad, void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  if (!x || !W || !y || !output || !row_loss || !loss || !correct || !inv_x || !inv_w || !lse || !tgrad || !shape_ok(B, N) ||
      !(eps > 0.f))
    return MA_ERR_INVALID_ARG;
  if (!width_ok(D)) return MA_ERR_UNSUPPORTED;
  if (((uintptr_t)x & 15) || ((uintptr_t)W & 15)) return MA_ERR_INVALID_ARG;
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < fwd_bytes(B, N)) return MA_ERR_WORKSPACE;
  const int64_t nblk = (N + 31) / 32;
  const int64_t pb = round_up(B * nblk * 4, 256);
  char* ws = static_cast<char*>(workspace);
  float* pmax = reinterpret_cast<float*>(ws);
  float* psum = reinterpret_cast<float*>(ws + pb);
  int32_t* parg = reinterpret_cast<int32_t*>(ws + 2 * pb);
  float* tout = reinterpret_cast<float*>(ws + 3 * pb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Margin mg = make_margin(margin, easy_margin);
  MA_LAUNCH(aam_norms_kernel, dim3((unsigned)((B + N + 3) / 4)), dim3(256), 0, st, x, B, W, N, (int)D, eps, inv_x, inv_w);
  MA_LAUNCH(aam_fwd_kernel, dim3((unsigned)((N + FT - 1) / FT), (unsigned)((B + FT - 1) / FT)), dim3(256), 0, st, x, W, y,
            (const float*)inv_x, (const float*)inv_w, B, N, (int)D, scale, mg, output, pmax, psum, parg, tout, tgrad, nblk);
  MA_LAUNCH(aam_fwd_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, st, (const float*)pmax, (const float*)psum, (const int32_t*)parg,
            (const float*)tout, y, B, N, nblk, lse, row_loss, loss, correct);
  return MA_OK;
}

int ma_aam_softmax_bwd_f32(const float* x, const float* W, const int32_t* y, int64_t B, int32_t D, int64_t N, float scale, float eps,
                           const float* output, const float* inv_x, const float* inv_w, const float* lse, const float* tgrad,
                           const float* grad_scale, float l2, float* dx, float* dW, void* workspace, int64_t workspace_bytes,
                           ma_stream_t stream) {
  if (!x || !W || !y || !output || !inv_x || !inv_w || !lse || !tgrad || !grad_scale || !dx || !dW || !shape_ok(B, N) || !(eps > 0.f))
    return MA_ERR_INVALID_ARG;
  if (!width_ok(D)) return MA_ERR_UNSUPPORTED;
  if (((uintptr_t)x & 15) || ((uintptr_t)W & 15)) return MA_ERR_INVALID_ARG;
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < bwd_bytes(B, D, N)) return MA_ERR_WORKSPACE;
  int64_t slab, S;
  slabs_of(B, N, &slab, &S);
  float* part = static_cast<float*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  MA_LAUNCH(aam_bwd_gemm_kernel<false>, dim3((unsigned)((N + BM - 1) / BM), 1), dim3(256), 0, st, output, lse, tgrad, y, x, inv_x,
            grad_scale, scale, B, N, (int)D, (int64_t)0, dW);
  MA_LAUNCH(aam_bwd_gemm_kernel<true>, dim3((unsigned)((B + BM - 1) / BM), (unsigned)S), dim3(256), 0, st, output, lse, tgrad, y, W,
            inv_w, grad_scale, scale, B, N, (int)D, slab, part);
  MA_LAUNCH(aam_bwd_finish_kernel, dim3((unsigned)((B + N + 3) / 4)), dim3(256), 0, st, x, W, inv_x, inv_w, B, N, (int)D, eps, l2,
            (const float*)part, S, dx, dW);
  return MA_OK;
}

int ma_aam_margin_f32(const float* cosine, const float* targets, int64_t n, float margin, float scale, int32_t easy_margin, float* out,
                      ma_stream_t stream) {
  if (!cosine || !targets || !out || n < 0 || n > (int64_t)0x7fffffff * 256) return MA_ERR_INVALID_ARG;
  if (n == 0) return MA_OK;
  MA_LAUNCH(aam_margin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), cosine, targets, n,
            scale, make_margin(margin, easy_margin), out);
  return MA_OK;
}

}  // extern "C"
