// CTC prefix beam search and attention rescoring (mindaudio/utils/recognize.py:273-406, models/decoders/decoder_factory.py:195-275)
// for gfx950.  The reference runs both searches as host Python loops (one utterance at a time, ~0.2 s per 10 s utterance on a CPU);
// here they are device work around the same encoder and decoder calls:
//   ctc_topk            TopK(log_softmax(logits), k): one wave per frame row, a sorted list of 16 per lane, merged across the wave
//   ctc_prefix_beam     the prefix search, one workgroup per utterance and frame after frame: the candidates of a frame are built
//                       in parallel (a thread per hypothesis key and per (top-k entry, hypothesis) child), ranked by counting, and
//                       the surviving prefixes copied into the other half of a double-buffered token array in LDS
//   hyp_score           sum of the decoder's log-probabilities along each hypothesis + eos + ctc_weight * CTC score, best per
//                       utterance (a wave per decoder row for its logsumexp and pick, then one thread per utterance)
// Scores are float64 as the reference's Python floats, with its log_add (utils/common.py:128-136) in its argument order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kTkList = 16;                          // ma_ctc_topk_f32: k <= 16
constexpr int kBmMax = 16;                           // beam <= 16
constexpr int kBmCand = kBmMax + kBmMax * kBmMax;    // candidate slots: hypothesis keys | children (top-k entry e, hypothesis i)
constexpr int kBmTokLds = 144 * 1024;                // double-buffered prefix tokens (dynamic LDS)
constexpr uint64_t kBmHashMul = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ bool cb_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// One wave per row: logp = (x - max) - log(sum exp(x - max)) in float32, each lane keeps the 16 best (logp, index) of its columns in
// a sorted register list (columns visited in ascending order, so equal values keep the lower index first), then k rounds of a wave
// arg-max over the lanes' heads; the winning lane pops its head.
__global__ __launch_bounds__(256) void ctc_topk_kernel(const float* __restrict__ logits, int64_t ld, int64_t rows, int V, int k,
                                                       float* __restrict__ out_v, int32_t* __restrict__ out_i) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = logits + row * ld;
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, p[v]);
  m = wave_max(m);
  float s = 0.0f;
  for (int v = lane; v < V; v += 64) s += expf(p[v] - m);
  const float lse = logf(wave_sum(s));
  float val[kTkList];
  int idx[kTkList];
#pragma unroll
  for (int j = 0; j < kTkList; ++j) {
    val[j] = -INFINITY;
    idx[j] = 0x7fffffff;
  }
  for (int v = lane; v < V; v += 64) {
    float cv = (p[v] - m) - lse;
    int ci = v;
    if (!cb_better(cv, ci, val[kTkList - 1], idx[kTkList - 1])) continue;
#pragma unroll
    for (int j = 0; j < kTkList; ++j)
      if (cb_better(cv, ci, val[j], idx[j])) {
        const float tv = val[j];
        const int ti = idx[j];
        val[j] = cv;
        idx[j] = ci;
        cv = tv;
        ci = ti;
      }
  }
  for (int r = 0; r < k; ++r) {
    float bv = val[0];
    int bi = idx[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (cb_better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (idx[0] == bi) {  // (column indices are unique across the lanes; k <= V, so the winner is a real column)
#pragma unroll
      for (int j = 0; j < kTkList - 1; ++j) {
        val[j] = val[j + 1];
        idx[j] = idx[j + 1];
      }
      val[kTkList - 1] = -INFINITY;
      idx[kTkList - 1] = 0x7fffffff;
    }
    if (lane == 0) {
      out_v[row * k + r] = bv;
      out_i[row * k + r] = bi;
    }
  }
}

// log_add (utils/common.py:128-136): -inf when every argument is -inf, else max + log(sum(exp(a - max))) summed left to right
__device__ __forceinline__ double cb_log_add2(double a, double b) {
  if (a == -INFINITY && b == -INFINITY) return -INFINITY;
  const double m = fmax(a, b);
  double s = 0.0;
  s += exp(a - m);
  s += exp(b - m);
  return m + log(s);
}
__device__ __forceinline__ double cb_log_add3(double a, double b, double c) {
  if (a == -INFINITY && b == -INFINITY && c == -INFINITY) return -INFINITY;
  const double m = fmax(fmax(a, b), c);
  double s = 0.0;
  s += exp(a - m);
  s += exp(b - m);
  s += exp(c - m);
  return m + log(s);
}

// One workgroup (256 threads) per utterance.  The reference's frame step (recognize.py:296-333) touches, for top-k entry e (outer
// loop) and hypothesis i (inner loop), the key `prefix_i` (blank, or s == last_i) and / or the key `prefix_i + s` (s == last_i: after
// prefix_i; else alone), and ranks the keys by log_add(pb, pnb) with ties in first-touch order (a stable sort over a defaultdict).
// A touch is event (e, i, sub) with position (e * 16 + i) * 2 + sub.  Keys come in two kinds:
//   - a hypothesis j of the beam (slot j): pb from the blank entry only (top-k indices are distinct), pnb from at most two touches,
//     both at the entry e = position of last_j: j's own repeat (s == last_j) and the child (parent(j), last_j), where parent(j) is
//     the hypothesis equal to prefix_j[:-1] if the beam holds it - applied in event order;
//   - a new child (i, s) that equals no hypothesis (slot 16 + e * 16 + i): touched once.
// Distinct keys never share an event, so the first-touch positions are distinct and (score desc, position asc) is a total order:
// a candidate's rank = the number of candidates before it.
__global__ __launch_bounds__(256) void ctc_prefix_beam_kernel(const float* __restrict__ topk_logp, const int32_t* __restrict__ topk_index,
                                                              const float* __restrict__ mask, int T, int beam, int blank,
                                                              int32_t* __restrict__ hyp, int32_t* __restrict__ hyp_len,
                                                              double* __restrict__ score, int32_t* __restrict__ n_hyp) {
  extern __shared__ __attribute__((aligned(16))) int32_t cb_tok[];  // [2][beam][T]
  __shared__ double h_pb[2][kBmMax], h_pnb[2][kBmMax];
  __shared__ uint64_t h_hash[2][kBmMax], h_phash[2][kBmMax];  // hash of the prefix, of the prefix without its last token
  __shared__ int h_len[2][kBmMax], h_last[2][kBmMax];
  __shared__ int h_par[kBmMax];
  __shared__ double c_pb[kBmCand], c_pnb[kBmCand], c_score[kBmCand];
  __shared__ int c_pos[kBmCand];  // first-touch position, -1 = no candidate
  __shared__ float f_lp[kBmMax];
  __shared__ int f_ix[kBmMax];
  __shared__ int n_sel[kBmMax];
  __shared__ int s_nh, s_nn;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t fb = (int64_t)b * T;
  int cur = 0;
  if (tid == 0) {  // cur_hyps = [((), (0.0, -inf))]
    s_nh = 1;
    h_pb[0][0] = 0.0;
    h_pnb[0][0] = -INFINITY;
    h_hash[0][0] = 0;
    h_phash[0][0] = 0;
    h_len[0][0] = 0;
    h_last[0][0] = -1;  // (None: equals no top-k index)
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    if (mask && mask[fb + t] == 0.0f) continue;  // (block-uniform)
    const int nh = s_nh;
    const int32_t* tc = cb_tok + (int64_t)cur * beam * T;
    int32_t* tn = cb_tok + (int64_t)(cur ^ 1) * beam * T;
    if (tid < beam) {
      f_lp[tid] = topk_logp[(fb + t) * beam + tid];
      f_ix[tid] = topk_index[(fb + t) * beam + tid];
    }
    if (tid == 0) s_nn = 0;
    // parent(j): the hypothesis i with len_i == len_j - 1 and prefix_i == prefix_j[:-1] (hash filter, then an exact compare by the wave)
    for (int j = wave; j < nh; j += 4) {
      const int lj = h_len[cur][j];
      int par = -1;
      if (lj > 0) {
        const bool cand = lane < nh && h_len[cur][lane] == lj - 1 && h_hash[cur][lane] == h_phash[cur][j];
        uint64_t bal = __ballot(cand);
        while (bal && par < 0) {
          const int i = __ffsll((unsigned long long)bal) - 1;
          bal &= bal - 1;
          int diff = 0;
          for (int x = lane; x < lj - 1; x += 64) diff |= tc[i * T + x] != tc[j * T + x];
          if (!__any(diff)) par = i;
        }
      }
      if (lane == 0) h_par[j] = par;
    }
    __syncthreads();
    for (int c = tid; c < kBmCand; c += 256) {
      int pos = -1;
      double npb = -INFINITY, npnb = -INFINITY;
      if (c < kBmMax) {  // hypothesis key j
        const int j = c;
        if (j < nh) {
          const int lastj = h_last[cur][j];
          int eb = -1, el = -1;
          for (int e = 0; e < beam; ++e) {
            if (f_ix[e] == blank) eb = e;
            else if (f_ix[e] == lastj) el = e;
          }
          const double pb = h_pb[cur][j], pnb = h_pnb[cur][j];
          int first = 0x7fffffff;
          if (eb >= 0) {
            const double ps = (double)f_lp[eb];
            npb = cb_log_add3(-INFINITY, pb + ps, pnb + ps);
            first = (eb * kBmMax + j) * 2;
          }
          if (el >= 0) {
            const double ps = (double)f_lp[el];
            const int rj = (el * kBmMax + j) * 2;
            first = min(first, rj);
            const int p = h_par[j];
            if (p >= 0) {
              const bool prep = h_last[cur][p] == lastj;  // the parent's own repeat branch: the child is its second touch
              const int rp = (el * kBmMax + p) * 2 + (prep ? 1 : 0);
              first = min(first, rp);
              const double ppb = h_pb[cur][p], ppnb = h_pnb[cur][p];
              if (rp < rj) {
                npnb = prep ? cb_log_add2(npnb, ppb + ps) : cb_log_add3(npnb, ppb + ps, ppnb + ps);
                npnb = cb_log_add2(npnb, pnb + ps);
              } else {
                npnb = cb_log_add2(npnb, pnb + ps);
                npnb = prep ? cb_log_add2(npnb, ppb + ps) : cb_log_add3(npnb, ppb + ps, ppnb + ps);
              }
            } else {
              npnb = cb_log_add2(npnb, pnb + ps);
            }
          }
          if (first != 0x7fffffff) pos = first;
        }
      } else {  // child (i, s) of top-k entry e, unless it is a hypothesis of the beam
        const int e = (c - kBmMax) / kBmMax, i = (c - kBmMax) % kBmMax;
        if (e < beam && i < nh) {
          const int s = f_ix[e];
          bool merged = s == blank;
          for (int j = 0; j < nh; ++j) merged |= h_par[j] == i && h_last[cur][j] == s;
          if (!merged) {
            const double ps = (double)f_lp[e];
            const bool rep = s == h_last[cur][i];
            npnb = rep ? cb_log_add2(-INFINITY, h_pb[cur][i] + ps) : cb_log_add3(-INFINITY, h_pb[cur][i] + ps, h_pnb[cur][i] + ps);
            pos = (e * kBmMax + i) * 2 + (rep ? 1 : 0);
          }
        }
      }
      c_pos[c] = pos;
      c_pb[c] = npb;
      c_pnb[c] = npnb;
      c_score[c] = cb_log_add2(npb, npnb);
    }
    __syncthreads();
    for (int c = tid; c < kBmCand; c += 256) {
      const int pc = c_pos[c];
      if (pc < 0) continue;
      const double sc = c_score[c];
      int rank = 0;
      for (int o = 0; o < kBmCand; ++o) {
        const int po = c_pos[o];
        const double so = c_score[o];
        rank += po >= 0 && (so > sc || (so == sc && po < pc));
      }
      if (rank < beam) {
        n_sel[rank] = c;
        atomicMax(&s_nn, rank + 1);  // the ranks are 0 .. n - 1: the new beam holds min(n, beam)
      }
    }
    __syncthreads();
    const int nn = s_nn;
    const int nxt = cur ^ 1;
    if (tid < nn) {
      const int c = n_sel[tid];
      const int src = c < kBmMax ? c : (c - kBmMax) % kBmMax;
      const int app = c < kBmMax ? -1 : f_ix[(c - kBmMax) / kBmMax];
      h_pb[nxt][tid] = c_pb[c];
      h_pnb[nxt][tid] = c_pnb[c];
      h_len[nxt][tid] = h_len[cur][src] + (app >= 0 ? 1 : 0);
      h_last[nxt][tid] = app >= 0 ? app : h_last[cur][src];
      h_hash[nxt][tid] = app >= 0 ? h_hash[cur][src] * kBmHashMul + (uint64_t)(uint32_t)(app + 1) : h_hash[cur][src];
      h_phash[nxt][tid] = app >= 0 ? h_hash[cur][src] : h_phash[cur][src];
    }
    for (int p = wave; p < nn; p += 4) {  // prefix tokens of the new beam (len <= frames seen <= T)
      const int c = n_sel[p];
      const int src = c < kBmMax ? c : (c - kBmMax) % kBmMax;
      const int app = c < kBmMax ? -1 : f_ix[(c - kBmMax) / kBmMax];
      const int ls = h_len[cur][src];
      for (int x = lane; x < ls; x += 64) tn[p * T + x] = tc[src * T + x];
      if (app >= 0 && lane == 0) tn[p * T + ls] = app;
    }
    __syncthreads();
    if (tid == 0) s_nh = nn;
    cur = nxt;
    __syncthreads();
  }
  const int nh = s_nh;
  const int32_t* tc = cb_tok + (int64_t)cur * beam * T;
  for (int p = wave; p < beam; p += 4) {
    const int lp = p < nh ? h_len[cur][p] : 0;
    int32_t* dst = hyp + ((int64_t)b * beam + p) * T;
    for (int x = lane; x < T; x += 64) dst[x] = x < lp ? tc[p * T + x] : 0;
    if (lane == 0) {
      hyp_len[(int64_t)b * beam + p] = lp;
      score[(int64_t)b * beam + p] = p < nh ? cb_log_add2(h_pb[cur][p], h_pnb[cur][p]) : -INFINITY;
    }
  }
  if (tid == 0) n_hyp[b] = nh;
}
MA_LDS_ATTR(ctc_prefix_beam_kernel, kBmTokLds);

// hyp_score, launch 1: one wave per decoder row (hypothesis h, position j <= len_h): the row's log-probability of its token (tok_j,
// or eos at j == len_h).  The logsumexp is float32 max + float64 sum of the float32 exponentials.
__global__ __launch_bounds__(256) void hyp_term_kernel(const float* __restrict__ logits, int64_t ld, int V, int64_t nrows, int group,
                                                       int L1, const int32_t* __restrict__ tokens, int64_t ld_tok,
                                                       const int32_t* __restrict__ lens, const int32_t* __restrict__ n_hyp, int eos,
                                                       double* __restrict__ terms) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const int64_t h = row / L1;
  const int j = (int)(row % L1);
  const int len = lens[h];
  if (n_hyp && (int)(h % group) >= n_hyp[h / group]) return;
  if (len < 0 || len > L1 - 1 || j > len) return;
  const int tok = j < len ? tokens[h * ld_tok + j] : eos;
  const float* p = logits + row * ld;
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, p[v]);
  m = wave_max(m);
  double s = 0.0;
  for (int v = lane; v < V; v += 64) s += (double)expf(p[v] - m);
  s = wave_sum(s);
  if (lane == 0) terms[row] = (tok >= 0 && tok < V) ? ((double)p[tok] - (double)m) - log(s) : NAN;
}

// hyp_score, launch 2: one thread per utterance - each hypothesis' sum in the reference's order, then the first best (`>`)
__global__ void hyp_pick_kernel(const double* __restrict__ terms, int64_t n_utt, int group, int L1, const int32_t* __restrict__ lens,
                                const int32_t* __restrict__ n_hyp, const double* __restrict__ ctc_score, double ctc_weight,
                                double* __restrict__ hyp_score, int32_t* __restrict__ best_index, double* __restrict__ best_score) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_utt) return;
  const int nv = n_hyp ? n_hyp[b] : group;
  double best = -INFINITY;
  int bi = 0;
  for (int g = 0; g < group; ++g) {
    const int64_t h = b * group + g;
    double sc = -INFINITY;
    if (g < nv) {
      const int len = lens[h];
      if (len < 0 || len > L1 - 1) {
        sc = NAN;
      } else {
        sc = 0.0;
        for (int j = 0; j <= len; ++j) sc += terms[h * L1 + j];
        sc += __dmul_rn(ctc_score[h], ctc_weight);  // (no contraction into an FMA: the reference rounds the product)
      }
      if (sc > best) {
        best = sc;
        bi = g;
      }
    }
    hyp_score[h] = sc;
  }
  best_index[b] = bi;
  best_score[b] = best;
}

}  // namespace ma

using namespace ma;

extern "C" {

int ma_ctc_topk_f32(const float* logits, int64_t ld, int64_t rows, int32_t V, int32_t k, float* topk_logp, int32_t* topk_index,
                    ma_stream_t stream) {
  if (!logits || !topk_logp || !topk_index || rows < 1 || V < 1 || ld < V || k < 1 || k > V) return MA_ERR_INVALID_ARG;
  if (k > kTkList) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(ctc_topk_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, ld, rows, (int)V, (int)k,
            topk_logp, topk_index);
  return MA_OK;
}

int ma_ctc_prefix_beam_search_f32(const float* topk_logp, const int32_t* topk_index, const float* mask, int64_t batch, int32_t T,
                                  int32_t beam, int32_t blank, int32_t* hyp, int32_t* hyp_len, double* score, int32_t* n_hyp,
                                  ma_stream_t stream) {
  if (!topk_logp || !topk_index || !hyp || !hyp_len || !score || !n_hyp || batch < 1 || batch > 0x7fffffff || T < 1 || beam < 1 ||
      blank < 0)
    return MA_ERR_INVALID_ARG;
  if (beam > kBmMax || (int64_t)2 * beam * T * 4 > kBmTokLds) return MA_ERR_UNSUPPORTED;
  const int lds = 2 * beam * T * 4;
  MA_LAUNCH(ctc_prefix_beam_kernel, dim3((unsigned)batch), dim3(256), lds, (hipStream_t)stream, topk_logp, topk_index, mask, (int)T,
            (int)beam, (int)blank, hyp, hyp_len, score, n_hyp);
  return MA_OK;
}

int ma_hyp_score_f32(const float* logits, int64_t ld, int32_t V, int64_t n_utt, int32_t group, int32_t L1, const int32_t* tokens,
                     int64_t ld_tok, const int32_t* lens, const int32_t* n_hyp, int32_t eos, const double* ctc_score,
                     double ctc_weight, double* workspace, double* hyp_score, int32_t* best_index, double* best_score,
                     ma_stream_t stream) {
  if (!logits || !tokens || !lens || !ctc_score || !workspace || !hyp_score || !best_index || !best_score) return MA_ERR_INVALID_ARG;
  if (V < 1 || ld < V || n_utt < 1 || group < 1 || L1 < 1 || ld_tok < L1 - 1 || eos < 0 || eos >= V) return MA_ERR_INVALID_ARG;
  const int64_t nrows = n_utt * group * L1;
  hipStream_t s = (hipStream_t)stream;
  MA_LAUNCH(hyp_term_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s, logits, ld, (int)V, nrows, (int)group, (int)L1,
            tokens, ld_tok, lens, n_hyp, (int)eos, workspace);
  MA_LAUNCH(hyp_pick_kernel, dim3((unsigned)((n_utt + 63) / 64)), dim3(64), 0, s, workspace, n_utt, (int)group, (int)L1, lens, n_hyp,
            ctc_score, ctc_weight, hyp_score, best_index, best_score);
  return MA_OK;
}

}  // extern "C"
