// Speaker-verification scoring (examples/ECAPA-TDNN/speaker_verification_cosine.py: emb_mean, evaluate2) on gfx950.
//
//   ma_cohort_stats_f32      mean / population std of the K largest cos(Q[e], C[n]) over n, per query row e  (the hot path)
//   ma_trial_scores_f32      cos(enrol, test) per trial, z- / t- / s-normalised with the statistics above
//   ma_running_mean_sub_f32  emb_mean: Y[n] = X[n] - g_n with g_n the running mean, state carried between calls
//   ma_sentence_mean_norm_f32  InputNormalization(norm_type="sentence", std_norm=False)
//
// Cohort statistics, per block of R query rows (R = what the caller's workspace holds, 512 recommended):
//   1. cohort_scores_kernel: S (R, N) float32 = exact-float32 MFMA product (v_mfma_f32_32x32x2_f32, 128 x 128 tiles, k in chunks of
//      32 through LDS) of the RAW rows, scaled in the epilogue by the float64 inverse norms of both sides and rounded once.
//   2. cohort_select_kernel: one workgroup per row.  Scores -> order-preserving 32-bit keys; most-significant-first radix select
//      (11 / 11 / 10 bits, integer LDS histograms) of the K-th largest key; the sums run over the strictly greater values plus
//      (K - count_greater) copies of the threshold, so that boundary ties give the sum NumPy's partition gives whichever tied
//      element it took.  The third histogram pass doubles as the summing pass (three reads of the row, not four).  Sums are
//      float64 of (x - t0), per-thread in index order then a fixed reduction: no floating-point atomics, two runs give identical
//      bits.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_common.h"
#include "launch.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int TM = 128;           // query rows per score tile
constexpr int TN = 128;           // cohort rows per score tile
constexpr int TK = 32;            // k per LDS chunk
constexpr int LDT = 160;          // LDS row stride (floats): lanes 32..63 read k + 1, 160 % 64 = 32 puts them on the other 32 banks
constexpr int SEL_THREADS = 1024;  // also the bin count of the select's last histogram
constexpr int ROWS_PER_SCAN_CHUNK = 256;

// 1 / ||x[r]|| in float64 (0 for a zero row: sklearn's normalize leaves such a row at zero); one wave per row
__global__ __launch_bounds__(256) void inv_norm_kernel(const float* __restrict__ x, int64_t ld, int64_t rows, int D,
                                                       double* __restrict__ inv) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)x[r * ld + d];
    s += v * v;
  }
  s = ma::wave_sum(s);
  if (lane == 0) inv[r] = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
}

// S[r - q0][n] = float(dot(Q[r], C[n]) * invq[r] * invc[n]) for r in [q0, q0 + rows), n in [0, N).
// grid (ceil(rows / TM), ceil(N / TN)): the query tiles of one cohort tile are neighbours, so the cohort streams from HBM once.
__global__ __launch_bounds__(256) void cohort_scores_kernel(const float* __restrict__ Q, int64_t ldq, const float* __restrict__ C,
                                                            int64_t ldc, const double* __restrict__ invq,
                                                            const double* __restrict__ invc, int64_t q0, int rows, int64_t N, int D,
                                                            float* __restrict__ S, int64_t lds) {
  __shared__ float As[TK * LDT];
  __shared__ float Bs[TK * LDT];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.x * TM;             // local query row of the tile
  const int64_t n0 = (int64_t)blockIdx.y * TN;
  const int lr = tid & 127, lh = tid >> 7;    // loader: row of the tile, which half of the 8 float4 of a 32-float chunk
  // Rows past the end of either matrix are read from the tile's first row instead (always inside): a tile row only feeds its own
  // outputs, and those are never stored.  (Selecting between a load and zeros makes the compiler load through flat pointers, whose
  // lgkmcnt waits then serialise the LDS reads of the MFMA loop behind the prefetch.)
  const float* ap = Q + (q0 + m0 + (m0 + lr < rows ? lr : 0)) * ldq;
  const float* bp = C + (n0 + (n0 + lr < N ? lr : 0)) * ldc;
  __shared__ double sq[TM];  // 1 / ||q|| of the tile's rows for the epilogue
  if (tid < TM) sq[tid] = m0 + tid < rows ? invq[q0 + m0 + tid] : 0.0;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 pa[4], pb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = lh + 2 * j;
    pa[j] = *reinterpret_cast<const float4*>(ap + 4 * q);
    pb[j] = *reinterpret_cast<const float4*>(bp + 4 * q);
  }
  const int chunks = D / TK;
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 4 * (lh + 2 * j);
      As[(k + 0) * LDT + lr] = pa[j].x;
      As[(k + 1) * LDT + lr] = pa[j].y;
      As[(k + 2) * LDT + lr] = pa[j].z;
      As[(k + 3) * LDT + lr] = pa[j].w;
      Bs[(k + 0) * LDT + lr] = pb[j].x;
      Bs[(k + 1) * LDT + lr] = pb[j].y;
      Bs[(k + 2) * LDT + lr] = pb[j].z;
      Bs[(k + 3) * LDT + lr] = pb[j].w;
    }
    __syncthreads();
    if (c + 1 < chunks) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = lh + 2 * j;
        pa[j] = *reinterpret_cast<const float4*>(ap + (c + 1) * TK + 4 * q);
        pb[j] = *reinterpret_cast<const float4*>(bp + (c + 1) * TK + 4 * q);
      }
    }
    const float* a_l = As + (lane >> 5) * LDT + wm * 64 + (lane & 31);
    const float* b_l = Bs + (lane >> 5) * LDT + wn * 64 + (lane & 31);
    // An MFMA accumulator is a k-ordered fmaf chain, and a chain's rounding error grows with its length (about 2e-7 of |q||c| at
    // D = 512 as one chain).  Each 32-deep chunk therefore starts its own chain from zero and is added to the running total once:
    // chains of 32 + D / 32 additions instead of one of D.
    f32x16 part[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[i][j][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < TK / 2; ++kk) {
      const float a0 = a_l[2 * kk * LDT], a1 = a_l[2 * kk * LDT + 32];
      const float b0 = b_l[2 * kk * LDT], b1 = b_l[2 * kk * LDT + 32];
      part[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, part[0][0], 0, 0, 0);
      part[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, part[0][1], 0, 0, 0);
      part[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, part[1][0], 0, 0, 0);
      part[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, part[1][1], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] += part[i][j];
  }
  // C/D map of the 32x32 forms: column = lane & 31 (cohort), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (query)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t n = n0 + wn * 64 + j * 32 + (lane & 31);
    if (n >= N) continue;
    const double ic = invc[n];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ml = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m0 + ml < rows) S[(int64_t)(m0 + ml) * lds + n] = (float)((double)acc[i][j][r] * sq[ml] * ic);
      }
    }
  }
}

__device__ __forceinline__ uint32_t order_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Wave 0: the bin holding the kk-th largest (1-based) candidate of hist[0 .. nbins), and how many candidates lie in higher bins.
__device__ void find_bin(const uint32_t* hist, int nbins, uint32_t kk, uint32_t* out_bin, uint32_t* out_above) {
  const int lane = threadIdx.x;  // caller guarantees threadIdx.x < 64
  const int per = nbins / 64;
  const int hi = nbins - lane * per;  // this lane owns bins [hi - per, hi), lane 0 the highest
  uint32_t s = 0;
  for (int b = 0; b < per; ++b) s += hist[hi - 1 - b];
  uint32_t p = s;  // inclusive prefix over lanes (higher bins first)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(p, o, 64);
    if (lane >= o) p += v;
  }
  const uint32_t ex = p - s;
  if (ex < kk && p >= kk) {  // exactly one lane
    uint32_t c = ex;
    for (int b = hi - 1; b >= hi - per; --b) {
      const uint32_t h = hist[b];
      if (c + h >= kk) {
        *out_bin = (uint32_t)b;
        *out_above = c;
        break;
      }
      c += h;
    }
  }
}

__global__ __launch_bounds__(SEL_THREADS) void cohort_select_kernel(const float* __restrict__ S, int64_t lds, int64_t N, int64_t K,
                                                                    double* __restrict__ mean, double* __restrict__ stdev) {
  __shared__ uint32_t hist[2048];
  __shared__ uint32_t s_bin, s_above;
  __shared__ double red[2][SEL_THREADS / 64];
  const float* row = S + (int64_t)blockIdx.x * lds;
  const int tid = threadIdx.x;
  const int64_t N4 = N >> 2;
  const float4* row4 = reinterpret_cast<const float4*>(row);  // lds % 4 == 0 and the block is 16-byte aligned

  uint32_t kk = (uint32_t)K;  // rank still to find among the candidates
  uint32_t prefix = 0;
  // pass p: candidates = keys whose bits above `shift + bits` equal prefix; histogram of their next `bits` bits.
  // The last pass also sums the values ABOVE the candidates' 22-bit prefix, as (x - t0) and (x - t0)^2 with t0 the smallest value
  // the prefix can hold; its 1024 bins are then single float values, so the candidates above the threshold are summed from their
  // counts.  That saves a fourth read of the row (the measured difference is in DESIGN.md).
  double s1 = 0.0, s2 = 0.0;
  double t0 = 0.0;
  for (int pass = 0; pass < 3; ++pass) {
    const int bits = pass < 2 ? 11 : 10;
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const uint32_t mask = (1u << bits) - 1u;
    for (int b = tid; b < 2048; b += SEL_THREADS) hist[b] = 0;
    __syncthreads();
    if (pass == 2) t0 = (double)key_value(prefix << 10);
    for (int64_t i = tid; i < N4; i += SEL_THREADS) {
      const float4 v = row4[i];
      const uint32_t k0 = order_key(v.x), k1 = order_key(v.y), k2 = order_key(v.z), k3 = order_key(v.w);
      if (pass == 0) {  // everything is a candidate; neighbours mostly share the bin: one LDS atomic for equal runs
        const uint32_t b0 = k0 >> 21, b1 = k1 >> 21, b2 = k2 >> 21, b3 = k3 >> 21;
        if (b0 == b1 && b1 == b2 && b2 == b3) {
          atomicAdd(&hist[b0], 4u);
        } else {
          atomicAdd(&hist[b0], 1u);
          atomicAdd(&hist[b1], 1u);
          atomicAdd(&hist[b2], 1u);
          atomicAdd(&hist[b3], 1u);
        }
      } else if (pass == 1) {
        if ((k0 >> 21) == prefix) atomicAdd(&hist[(k0 >> 10) & mask], 1u);
        if ((k1 >> 21) == prefix) atomicAdd(&hist[(k1 >> 10) & mask], 1u);
        if ((k2 >> 21) == prefix) atomicAdd(&hist[(k2 >> 10) & mask], 1u);
        if ((k3 >> 21) == prefix) atomicAdd(&hist[(k3 >> 10) & mask], 1u);
      } else {
        const uint32_t ks[4] = {k0, k1, k2, k3};
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const uint32_t hi = ks[c] >> 10;
          if (hi == prefix) {
            atomicAdd(&hist[ks[c] & mask], 1u);
          } else if (hi > prefix) {
            const double d = (double)e[c] - t0;
            s1 += d;
            s2 += d * d;
          }
        }
      }
    }
    for (int64_t i = 4 * N4 + tid; i < N; i += SEL_THREADS) {
      const float x = row[i];
      const uint32_t k = order_key(x);
      if (pass == 0 || (k >> (shift + bits)) == prefix) {
        atomicAdd(&hist[(k >> shift) & mask], 1u);
      } else if (pass == 2 && (k >> 10) > prefix) {
        const double d = (double)x - t0;
        s1 += d;
        s2 += d * d;
      }
    }
    __syncthreads();
    if (tid < 64) find_bin(hist, 1 << bits, kk, &s_bin, &s_above);
    __syncthreads();
    prefix = (prefix << bits) | s_bin;
    kk -= s_above;
    __syncthreads();  // s_bin / s_above are rewritten by the next pass
  }
  // prefix is the K-th largest key, kk (>= 1) how many copies of it belong to the K largest.  Bin b of the last histogram is the
  // single value key (prefix & ~1023) | b: thread b adds the bins above the threshold's.
  const uint32_t tbin = prefix & 1023u;
  if ((uint32_t)tid > tbin && hist[tid]) {  // SEL_THREADS == 1024 bins
    const double d = (double)key_value((prefix & ~1023u) | (uint32_t)tid) - t0;
    s1 += (double)hist[tid] * d;
    s2 += (double)hist[tid] * d * d;
  }
  s1 = ma::wave_sum(s1);
  s2 = ma::wave_sum(s2);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = s1;
    red[1][tid >> 6] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
    const double dt = (double)key_value(prefix) - t0;  // the threshold's kk copies
    a += (double)kk * dt;
    b += (double)kk * dt * dt;
    const double m = a / (double)K;
    double var = b / (double)K - m * m;
    if (var < 0.0) var = 0.0;
    mean[blockIdx.x] = t0 + m;
    stdev[blockIdx.x] = sqrt(var);
  }
}

// one wave per trial
__global__ __launch_bounds__(256) void trial_scores_kernel(const float* __restrict__ emb, int64_t ld, int64_t n_emb, int D,
                                                           const int32_t* __restrict__ enrol_idx,
                                                           const int32_t* __restrict__ test_idx, int64_t T,
                                                           const double* __restrict__ mean, const double* __restrict__ stdev,
                                                           int mode, double* __restrict__ score) {
  const int64_t tr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tr >= T) return;
  const int lane = threadIdx.x & 63;
  const int64_t ie = enrol_idx[tr], it = test_idx[tr];
  if (ie < 0 || ie >= n_emb || it < 0 || it >= n_emb) {  // never read outside the matrix; the wrapper checks the lists
    if (lane == 0) score[tr] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const float* e = emb + ie * ld;
  const float* u = emb + it * ld;
  double dot = 0.0, ne = 0.0, nt = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double a = (double)e[d], b = (double)u[d];
    dot += a * b;
    ne += a * a;
    nt += b * b;
  }
  dot = ma::wave_sum(dot);
  ne = ma::wave_sum(ne);
  nt = ma::wave_sum(nt);
  if (lane != 0) return;
  double s = (ne > 0.0 && nt > 0.0) ? dot / (sqrt(ne) * sqrt(nt)) : 0.0;
  if (mode == MA_SCORE_NORM_Z) {
    s = (s - mean[ie]) / stdev[ie];
  } else if (mode == MA_SCORE_NORM_T) {
    s = (s - mean[it]) / stdev[it];
  } else if (mode == MA_SCORE_NORM_S) {
    s = 0.5 * ((s - mean[ie]) / stdev[ie] + (s - mean[it]) / stdev[it]);
  }
  score[tr] = s;
}

// emb_mean's recurrence g_n = (1 - w) g_{n-1} + w x_n, w = 1 / (count + 1), is the cumulative mean
// g_n = (count0 * g_in + x_0 + ... + x_n) / (count0 + n + 1): a prefix sum over rows, columns independent.
// 1. column sums of each chunk of rows
__global__ void scan_chunk_sums_kernel(const float* __restrict__ X, int64_t ldx, int64_t N, int D, double* __restrict__ part) {
  const int d = threadIdx.x;
  if (d >= D) return;
  const int64_t r0 = (int64_t)blockIdx.x * ROWS_PER_SCAN_CHUNK;
  const int64_t r1 = r0 + ROWS_PER_SCAN_CHUNK < N ? r0 + ROWS_PER_SCAN_CHUNK : N;
  double s = 0.0;
  for (int64_t r = r0; r < r1; ++r) s += (double)X[r * ldx + d];
  part[(int64_t)blockIdx.x * D + d] = s;
}
// 2. one workgroup: part[c] <- count0 * g_in + sum of the chunks before c; g <- the mean after the last row
__global__ void scan_offsets_kernel(double* __restrict__ part, int64_t chunks, int D, double* __restrict__ g, int64_t count0,
                                    int64_t N) {
  const int d = threadIdx.x;
  if (d >= D) return;
  double run = count0 > 0 ? (double)count0 * g[d] : 0.0;
  for (int64_t c = 0; c < chunks; ++c) {
    const double s = part[c * D + d];
    part[c * D + d] = run;
    run += s;
  }
  g[d] = run / (double)(count0 + N);
}
// 3. the rows of each chunk
__global__ void scan_apply_kernel(const float* __restrict__ X, int64_t ldx, int64_t N, int D, const double* __restrict__ part,
                                  int64_t count0, float* __restrict__ Y, int64_t ldy) {
  const int d = threadIdx.x;
  if (d >= D) return;
  const int64_t r0 = (int64_t)blockIdx.x * ROWS_PER_SCAN_CHUNK;
  const int64_t r1 = r0 + ROWS_PER_SCAN_CHUNK < N ? r0 + ROWS_PER_SCAN_CHUNK : N;
  double run = part[(int64_t)blockIdx.x * D + d];
  for (int64_t r = r0; r < r1; ++r) {
    const double x = (double)X[r * ldx + d];
    run += x;
    Y[r * ldy + d] = (float)(x - run / (double)(count0 + r + 1));
  }
}

// x (batch, T, F) -> x - mean over T, per (utterance, feature); one workgroup per (utterance, 64 features), 4 time phases
__global__ __launch_bounds__(256) void sentence_mean_norm_kernel(const float* __restrict__ x, int64_t T, int F,
                                                                 float* __restrict__ out) {
  __shared__ double part[4][64];
  const int f = blockIdx.x * 64 + (threadIdx.x & 63);
  const int ph = threadIdx.x >> 6;
  const float* xb = x + (int64_t)blockIdx.y * T * F;
  float* ob = out + (int64_t)blockIdx.y * T * F;
  double s = 0.0;
  if (f < F)
    for (int64_t t = ph; t < T; t += 4) s += (double)xb[t * F + f];
  part[ph][threadIdx.x & 63] = s;
  __syncthreads();
  const int c = threadIdx.x & 63;
  const double m = (((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]) / (double)T;
  if (f < F)
    for (int64_t t = ph; t < T; t += 4) ob[t * F + f] = (float)((double)xb[t * F + f] - m);
}

bool width_ok(int32_t D) { return D >= 32 && D <= 512 && D % 32 == 0; }
constexpr int64_t kAlign = 256;
constexpr int64_t kBlockRows = 512;  // recommended query rows per pass: 14.1 ms at E = 4 708, N = 400 000 (256: 15.5, 1024: 13.7)
int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

}  // namespace

extern "C" {

int64_t ma_cohort_stats_workspace_bytes(int64_t E, int64_t N) {
  if (E < 1 || N < 1 || N > 0x7fffffff) return MA_ERR_INVALID_ARG;
  const int64_t rows = E < kBlockRows ? E : kBlockRows;
  return round_up(8 * E, kAlign) + round_up(8 * N, kAlign) + rows * round_up(N, 4) * 4;
}

int ma_cohort_stats_f32(const float* Q, int64_t ldq, const float* C, int64_t ldc, int64_t E, int64_t N, int32_t D, int64_t K,
                        double* mean, double* stdev, void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  if (!Q || !C || !mean || !stdev || E < 1 || N < 1 || N > 0x7fffffff || !width_ok(D) || K < 1 || K > N) return MA_ERR_INVALID_ARG;
  if (ldq < D || ldc < D || ldq % 4 || ldc % 4 || ((uintptr_t)Q & 15) || ((uintptr_t)C & 15)) return MA_ERR_INVALID_ARG;
  const int64_t lds = round_up(N, 4);
  const int64_t fixed = round_up(8 * E, kAlign) + round_up(8 * N, kAlign);
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < fixed + lds * 4) return MA_ERR_WORKSPACE;
  int64_t R = (workspace_bytes - fixed) / (lds * 4);
  if (R > E) R = E;
  if (R > 32768) R = 32768;
  double* invq = reinterpret_cast<double*>(workspace);
  double* invc = reinterpret_cast<double*>(static_cast<char*>(workspace) + round_up(8 * E, kAlign));
  float* S = reinterpret_cast<float*>(static_cast<char*>(workspace) + fixed);
  hipStream_t s = static_cast<hipStream_t>(stream);
  MA_LAUNCH(inv_norm_kernel, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, s, Q, ldq, E, (int)D, invq);
  MA_LAUNCH(inv_norm_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, C, ldc, N, (int)D, invc);
  const unsigned ny = (unsigned)((N + TN - 1) / TN);
  for (int64_t q0 = 0; q0 < E; q0 += R) {
    const int rows = (int)(E - q0 < R ? E - q0 : R);
    MA_LAUNCH(cohort_scores_kernel, dim3((unsigned)((rows + TM - 1) / TM), ny), dim3(256), 0, s, Q, ldq, C, ldc, invq, invc, q0,
              rows, N, (int)D, S, lds);
    MA_LAUNCH(cohort_select_kernel, dim3((unsigned)rows), dim3(SEL_THREADS), 0, s, S, lds, N, K, mean + q0, stdev + q0);
  }
  return MA_OK;
}

int ma_trial_scores_f32(const float* emb, int64_t ld, int64_t n_emb, int32_t D, const int32_t* enrol_idx, const int32_t* test_idx,
                        int64_t T, const double* mean, const double* stdev, int32_t mode, double* score, ma_stream_t stream) {
  if (!emb || !enrol_idx || !test_idx || !score || n_emb < 1 || n_emb > 0x7fffffff || T < 0 || !width_ok(D) || ld < D)
    return MA_ERR_INVALID_ARG;
  if (mode < MA_SCORE_NORM_NONE || mode > MA_SCORE_NORM_S) return MA_ERR_INVALID_ARG;
  if (mode != MA_SCORE_NORM_NONE && (!mean || !stdev)) return MA_ERR_INVALID_ARG;
  if (T == 0) return MA_OK;
  MA_LAUNCH(trial_scores_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), emb, ld, n_emb,
            (int)D, enrol_idx, test_idx, T, mean, stdev, (int)mode, score);
  return MA_OK;
}

int64_t ma_running_mean_sub_workspace_bytes(int64_t N, int32_t D) {
  if (N < 1 || !width_ok(D)) return MA_ERR_INVALID_ARG;
  return (N + ROWS_PER_SCAN_CHUNK - 1) / ROWS_PER_SCAN_CHUNK * D * 8;
}

int ma_running_mean_sub_f32(const float* X, int64_t ldx, int64_t N, int32_t D, double* g_mean, int64_t count, float* Y, int64_t ldy,
                            void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  if (!X || !Y || !g_mean || N < 1 || count < 0 || !width_ok(D) || ldx < D || ldy < D) return MA_ERR_INVALID_ARG;
  const int64_t chunks = (N + ROWS_PER_SCAN_CHUNK - 1) / ROWS_PER_SCAN_CHUNK;
  if (chunks > 0x7fffffff) return MA_ERR_INVALID_ARG;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < chunks * D * 8) return MA_ERR_WORKSPACE;
  double* part = static_cast<double*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  MA_LAUNCH(scan_chunk_sums_kernel, dim3((unsigned)chunks), dim3(D), 0, s, X, ldx, N, (int)D, part);
  MA_LAUNCH(scan_offsets_kernel, dim3(1), dim3(D), 0, s, part, chunks, (int)D, g_mean, count, N);
  MA_LAUNCH(scan_apply_kernel, dim3((unsigned)chunks), dim3(D), 0, s, X, ldx, N, (int)D, part, count, Y, ldy);
  return MA_OK;
}

int ma_sentence_mean_norm_f32(const float* x, int64_t batch, int64_t T, int32_t F, float* out, ma_stream_t stream) {
  if (!x || !out || batch < 1 || batch > 65535 || T < 1 || F < 1) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(sentence_mean_norm_kernel, dim3((unsigned)((F + 63) / 64), (unsigned)batch), dim3(256), 0,
            static_cast<hipStream_t>(stream), x, T, (int)F, out);
  return MA_OK;
}

}  // extern "C"
