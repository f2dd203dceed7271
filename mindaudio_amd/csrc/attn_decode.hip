// The autoregressive `attention` decode mode (mindaudio/utils/recognize.py:78-251, models/decoders/decoder_factory.py:59-192 and
// 278-413) for gfx950.  The reference re-runs the whole decoder on the maxlen-padded prefix at every step; here a step advances one
// token on a key / value cache and the beam bookkeeping never leaves the device:
//   decoder_self_attn_step   one query per (row, head) over the row's cached keys: one wave per (row, head), eight lanes per key
//                            (16 bytes each), the beam reorder (cache row of the parent) and the append in the same launch
//   attn_beam_step           steps 2.2-2.6 of the search: one workgroup per utterance, a thread per (row, top-k entry) candidate,
//                            ranked by counting, token rows gathered from the parents
//   attn_beam_best           topk_fun(scores, 1) and the winner's token row
// Nothing here is bound by the matrix pipe: a step reads (t + 1) * 256 bytes per (row, head) and is a chain of dependent launches,
// so the kernels are shaped for latency (no LDS staging of K / V, no atomics, no inter-workgroup hand-off).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kAdD = 64;         // d_k
constexpr int kAdMaxL = 2048;    // cached positions (float32 scores of one (row, head) in LDS)
constexpr int kAbMax = 16;       // beam <= 16 (ma_ctc_topk_f32's k)

__device__ __forceinline__ void ad_unpack8(const uint4 u, float (&f)[8]) {
  f[0] = bf2f_lo(u.x & 0xffffu); f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = bf2f_lo(u.y & 0xffffu); f[3] = __uint_as_float(u.y & 0xffff0000u);
  f[4] = bf2f_lo(u.z & 0xffffu); f[5] = __uint_as_float(u.z & 0xffff0000u);
  f[6] = bf2f_lo(u.w & 0xffffu); f[7] = __uint_as_float(u.w & 0xffff0000u);
}

// workgroup = one wave = (row r, head h), blockIdx.x = r * heads + h.  Lane (g = lane / 8, c = lane % 8): key j = 8 * i + g of pass i, elements 8 c .. 8 c + 7
// of the head.  Pass 1 copies the parent's K / V pieces into the out cache as it reads them (position t comes from qkv) and leaves
// the scaled score of key j in LDS; the softmax is the wave's; pass 2 reads V again (from v_in / qkv, never from what the launch
// writes) and sums p_j v_j per lane group, the eight groups are added in a fixed order.
__global__ __launch_bounds__(64) void decoder_self_attn_step_kernel(const uint16_t* __restrict__ qkv, int64_t ldqkv,
                                                                   const uint16_t* __restrict__ k_in, const uint16_t* __restrict__ v_in,
                                                                   const int32_t* __restrict__ parent, int R, int Lmax, int t, int d,
                                                                   float scale, uint16_t* __restrict__ ctx, int64_t ldc,
                                                                   uint16_t* __restrict__ k_out, uint16_t* __restrict__ v_out) {
  __shared__ float S[kAdMaxL];
  const int H = d / kAdD, h = blockIdx.x % H, r = blockIdx.x / H, lane = threadIdx.x, g = lane >> 3, c = lane & 7;
  int p = parent ? parent[r] : r;
  p = p < 0 ? 0 : (p >= R ? R - 1 : p);  // (a parent outside [0, R) is clamped: no read leaves the cache)
  const int col = h * kAdD + c * 8;
  const uint16_t* nq = qkv + (int64_t)r * ldqkv + col;
  float q[8];
  ad_unpack8(*reinterpret_cast<const uint4*>(nq), q);
  const int64_t src = (int64_t)p * Lmax * d + col, dst = (int64_t)r * Lmax * d + col;
  const int n = t + 1;
  for (int j = g; j < n; j += 8) {
    uint4 kk, vv;
    if (j < t) {
      kk = *reinterpret_cast<const uint4*>(k_in + src + (int64_t)j * d);
      vv = *reinterpret_cast<const uint4*>(v_in + src + (int64_t)j * d);
    } else {
      kk = *reinterpret_cast<const uint4*>(nq + d);
      vv = *reinterpret_cast<const uint4*>(nq + 2 * d);
    }
    *reinterpret_cast<uint4*>(k_out + dst + (int64_t)j * d) = kk;
    *reinterpret_cast<uint4*>(v_out + dst + (int64_t)j * d) = vv;
    float kf[8];
    ad_unpack8(kk, kf);
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(q[e], kf[e], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (c == 0) S[j] = s * scale;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = lane; j < n; j += 64) m = fmaxf(m, S[j]);
  m = wave_max(m);
  float sum = 0.0f;
  for (int j = lane; j < n; j += 64) {
    const float e = __expf(S[j] - m);  // (exactly 0 more than ~104 below the maximum)
    S[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  __syncthreads();
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = g; j < n; j += 8) {
    const float pj = bf16_round(S[j] * inv);  // (the probability is a bf16 operand of ma_mha_small_fwd_bf16's P V product)
    const uint4 vv = j < t ? *reinterpret_cast<const uint4*>(v_in + src + (int64_t)j * d) : *reinterpret_cast<const uint4*>(nq + 2 * d);
    float vf[8];
    ad_unpack8(vv, vf);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, vf[e], acc[e]);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[e] += __shfl_xor(acc[e], 8, 64);
    acc[e] += __shfl_xor(acc[e], 16, 64);
    acc[e] += __shfl_xor(acc[e], 32, 64);
  }
  if (g == 0) {
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (uint32_t)f2bf(acc[2 * e]) | ((uint32_t)f2bf(acc[2 * e + 1]) << 16);
    *reinterpret_cast<uint4*>(ctx + (int64_t)r * ldc + col) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// One workgroup (256 threads) per utterance: thread c < N * N is candidate (row c / N, top-k entry c % N).
__global__ __launch_bounds__(256) void attn_beam_step_kernel(const float* __restrict__ topk_logp, const int32_t* __restrict__ topk_index,
                                                            const float* __restrict__ scores_in, const int32_t* __restrict__ end_in,
                                                            const int32_t* __restrict__ tokens_in, int N, int W, int eos, int max_new,
                                                            int32_t* __restrict__ length, int32_t* __restrict__ done,
                                                            float* __restrict__ scores_out, int32_t* __restrict__ end_out,
                                                            int32_t* __restrict__ tokens_out, int32_t* __restrict__ parent,
                                                            int32_t* __restrict__ pred) {
  __shared__ float c_val[kAbMax * kAbMax];
  __shared__ int c_tok[kAbMax * kAbMax];
  __shared__ int s_sel[kAbMax];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)b * N;
  const int len = length[b];
  // (a length that leaves no room for the next token freezes the utterance too: no store leaves the token row)
  const bool frozen = done[b] != 0 || len < 0 || len >= max_new || len + 1 >= W;
  if (frozen) {
    if (tid < N) {
      scores_out[r0 + tid] = scores_in[r0 + tid];
      end_out[r0 + tid] = end_in[r0 + tid];
      parent[r0 + tid] = (int32_t)(r0 + tid);
      pred[r0 + tid] = eos;
    }
    for (int s = wave; s < N; s += 4)
      for (int x = lane; x < W; x += 64) tokens_out[(r0 + s) * W + x] = tokens_in[(r0 + s) * W + x];
    if (tid == 0 && done[b] == 0) done[b] = 1;
    return;
  }
  const int nc = N * N;
  if (tid < nc) {
    const int r = tid / N, j = tid % N;
    const bool fin = end_in[r0 + r] != 0;
    const float lp = topk_logp[(r0 + r) * N + j];
    // mask_finished_scores: a finished row keeps one branch at exactly +0 (the reference's logp * 0 is NaN for an infinite logp)
    const float mm = fin ? (j == 0 ? 0.0f : lp + (-10000.0f)) : lp;
    c_val[tid] = scores_in[r0 + r] + mm;
    c_tok[tid] = fin ? eos : topk_index[(r0 + r) * N + j];
  }
  __syncthreads();
  if (tid < nc) {
    float v = c_val[tid];
    v = v != v ? -INFINITY : v;  // (a NaN candidate ranks as -inf, so that the order stays total)
    int rank = 0;
    for (int o = 0; o < nc; ++o) {
      float w = c_val[o];
      w = w != w ? -INFINITY : w;
      rank += w > v || (w == v && o < tid);
    }
    if (rank < N) s_sel[rank] = tid;
  }
  __syncthreads();
  if (tid < N) {
    const int cnd = s_sel[tid];
    const int tok = c_tok[cnd];
    scores_out[r0 + tid] = c_val[cnd];
    parent[r0 + tid] = (int32_t)(r0 + cnd / N);
    pred[r0 + tid] = tok;
    end_out[r0 + tid] = tok == eos ? 1 : 0;
  }
  for (int s = wave; s < N; s += 4) {
    const int cnd = s_sel[s];
    const int64_t pr = r0 + cnd / N;
    const int tok = c_tok[cnd];
    for (int x = lane; x < W; x += 64) tokens_out[(r0 + s) * W + x] = x == len + 1 ? tok : tokens_in[pr * W + x];
  }
  if (tid == 0) {
    int all = 1;
    for (int s = 0; s < N; ++s) all &= c_tok[s_sel[s]] == eos;
    length[b] = len + 1;
    if (all || len + 1 >= max_new) done[b] = 1;
  }
}

// One wave per utterance: the first slot with the highest score, its token row without column 0.
__global__ __launch_bounds__(64) void attn_beam_best_kernel(const float* __restrict__ scores, const int32_t* __restrict__ tokens, int N,
                                                           int W, const int32_t* __restrict__ length, int32_t* __restrict__ best_hyp,
                                                           int32_t* __restrict__ best_len, float* __restrict__ best_score) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t r0 = (int64_t)b * N;
  int bi = 0;
  float bs = scores[r0];
  for (int s = 1; s < N; ++s) {
    const float v = scores[r0 + s];
    if (v > bs || (bs != bs && v == v)) {
      bs = v;
      bi = s;
    }
  }
  for (int x = lane; x < W - 1; x += 64) best_hyp[(int64_t)b * (W - 1) + x] = tokens[(r0 + bi) * W + 1 + x];
  if (lane == 0) {
    best_len[b] = length[b];
    best_score[b] = bs;
  }
}

static bool ad_overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

}  // namespace ma

using namespace ma;

extern "C" {

int ma_decoder_self_attn_step_bf16(const void* qkv, int64_t ldqkv, const void* k_in, const void* v_in, const int32_t* parent,
                                   int64_t R, int32_t Lmax, int32_t t, int32_t heads, int32_t d_k, int32_t d, float scale, void* ctx,
                                   int64_t ldc, void* k_out, void* v_out, ma_stream_t stream) {
  if (!qkv || !k_in || !v_in || !ctx || !k_out || !v_out) return MA_ERR_INVALID_ARG;
  if (R < 1 || R * heads > 0x7fffffff || heads < 1 || Lmax < 1 || t < 0 || t >= Lmax) return MA_ERR_INVALID_ARG;
  if (d_k != kAdD || d != heads * kAdD || Lmax > kAdMaxL) return MA_ERR_UNSUPPORTED;
  if (ldqkv < 3 * (int64_t)d || ldc < d) return MA_ERR_INVALID_ARG;
  if ((ldqkv & 7) || (ldc & 7)) return MA_ERR_UNSUPPORTED;  // 16-byte row pieces
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(k_in) | reinterpret_cast<uintptr_t>(v_in) |
       reinterpret_cast<uintptr_t>(ctx) | reinterpret_cast<uintptr_t>(k_out) | reinterpret_cast<uintptr_t>(v_out)) & 15)
    return MA_ERR_INVALID_ARG;
  const int64_t bytes = R * Lmax * (int64_t)d * 2;
  if (ad_overlap(k_in, k_out, bytes) || ad_overlap(v_in, v_out, bytes) || ad_overlap(k_in, v_out, bytes) ||
      ad_overlap(v_in, k_out, bytes) || ad_overlap(k_out, v_out, bytes))
    return MA_ERR_INVALID_ARG;
  MA_LAUNCH(decoder_self_attn_step_kernel, dim3((unsigned)(R * heads)), dim3(64), 0, (hipStream_t)stream, (const uint16_t*)qkv,
            ldqkv, (const uint16_t*)k_in, (const uint16_t*)v_in, parent, (int)R, (int)Lmax, (int)t, (int)d, scale, (uint16_t*)ctx, ldc,
            (uint16_t*)k_out, (uint16_t*)v_out);
  return MA_OK;
}

int ma_attn_beam_step_f32(const float* topk_logp, const int32_t* topk_index, const float* scores_in, const int32_t* end_in,
                          const int32_t* tokens_in, int64_t batch, int32_t beam, int32_t W, int32_t eos, int32_t max_new,
                          int32_t* length, int32_t* done, float* scores_out, int32_t* end_out, int32_t* tokens_out, int32_t* parent,
                          int32_t* pred, ma_stream_t stream) {
  if (!topk_logp || !topk_index || !scores_in || !end_in || !tokens_in || !length || !done || !scores_out || !end_out || !tokens_out ||
      !parent || !pred)
    return MA_ERR_INVALID_ARG;
  if (batch < 1 || batch * beam > 0x7fffffff || beam < 1 || W < 1 || eos < 0 || max_new < 0 || max_new > W - 1) return MA_ERR_INVALID_ARG;
  if (beam > kAbMax) return MA_ERR_UNSUPPORTED;
  const int64_t rows = batch * beam;
  if (ad_overlap(tokens_in, tokens_out, rows * W * 4) || ad_overlap(scores_in, scores_out, rows * 4) ||
      ad_overlap(end_in, end_out, rows * 4))
    return MA_ERR_INVALID_ARG;
  MA_LAUNCH(attn_beam_step_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, topk_logp, topk_index, scores_in, end_in,
            tokens_in, (int)beam, (int)W, (int)eos, (int)max_new, length, done, scores_out, end_out, tokens_out, parent, pred);
  return MA_OK;
}

int ma_attn_beam_best_f32(const float* scores, const int32_t* tokens, const int32_t* length, int64_t batch, int32_t beam, int32_t W,
                          int32_t* best_hyp, int32_t* best_len, float* best_score, ma_stream_t stream) {
  if (!scores || !tokens || !length || !best_hyp || !best_len || !best_score) return MA_ERR_INVALID_ARG;
  if (batch < 1 || batch * beam > 0x7fffffff || beam < 1 || W < 1) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(attn_beam_best_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, scores, tokens, (int)beam, (int)W, length,
            best_hyp, best_len, best_score);
  return MA_OK;
}

}  // extern "C"
