// WaveGrad (mindaudio/models/wavegrad/wavegrad_v190.py, examples/wavegrad/reverse.py): everything between its MFMA products, and the
// host loops that chain them.  Contract: include/mindaudio_amd.h.  The products themselves are ma_conv1d_taps_bf16 / ma_gemm_bf16
// calls (gemm_bf16.hip), reached through their C entry points.
//
// wg_init_conv_kernel: one thread per (sample, 4 channels); the taps are an fma chain from the bias, float32 weights (taps, C0).
// wg_pack_kernel: one thread per (operand row, 8 channels): two 16-byte loads of x (and of shift, scale, enc), one 16-byte bf16 store;
//   halo rows and pad columns are stored as zeros by the same threads, so a call rewrites the whole operand buffer.
// wg_last_conv_kernel: one workgroup per 64 output samples of one utterance.  Each wave takes rows of x (C floats, 16 bytes a lane),
//   forms the `taps` dot products of the row against w (taps, C) and reduces them over the wave into LDS; 64 threads then add the
//   taps of their sample in tap order and apply the diffusion update.  x is read once.
// All three are bandwidth-bound; there is no device sin / cos / exp (the positional encodings are host tables).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kWgThreads = 256;
constexpr int kWgMaxTaps = 7;
constexpr int kWgLastRows = 64;
constexpr float kWgInvSqrt2 = 0.70710678118654752440f;

__global__ __launch_bounds__(kWgThreads) void wg_init_conv_kernel(const float* __restrict__ audio, int64_t T, const float* __restrict__ wt,
                                                                  const float* __restrict__ bias, int taps, int C0,
                                                                  float* __restrict__ out, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
  if (idx >= total) return;
  const int c4n = C0 >> 2;
  const int c = (int)(idx % c4n) * 4;
  const int64_t row = idx / c4n;  // b * T + t
  const int64_t b = row / T, t = row - b * T;
  f32x4 acc = *reinterpret_cast<const f32x4*>(bias + c);
  const int half = taps >> 1;
  for (int j = 0; j < taps; ++j) {
    const int64_t tt = t + j - half;
    const float a = (tt >= 0 && tt < T) ? audio[b * T + tt] : 0.0f;  // never the neighbouring utterance
    const f32x4 w = *reinterpret_cast<const f32x4*>(wt + (int64_t)j * C0 + c);
    acc.x = fmaf(a, w.x, acc.x);
    acc.y = fmaf(a, w.y, acc.y);
    acc.z = fmaf(a, w.z, acc.z);
    acc.w = fmaf(a, w.w, acc.w);
  }
  *reinterpret_cast<f32x4*>(out + row * C0 + c) = acc;
}

__global__ __launch_bounds__(kWgThreads) void wg_pack_kernel(const float* __restrict__ x, int64_t T_in, int64_t T_out, int f, int C, int Cpad,
                                                             int halo, const float* __restrict__ film, int64_t ld_film,
                                                             const float* __restrict__ enc, int64_t ld_enc, float slope, float mul,
                                                             uint16_t* __restrict__ out, float* __restrict__ res, float res_mul,
                                                             int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
  if (idx >= total) return;
  const int c8n = Cpad >> 3;
  const int c = (int)(idx % c8n) * 8;
  const int64_t row = idx / c8n;  // b * (T_out + 2 halo) + r
  const int64_t rows_u = T_out + 2 * (int64_t)halo;
  const int64_t b = row / rows_u, t = row - b * rows_u - halo;
  u32x4 o = {0u, 0u, 0u, 0u};
  if (t >= 0 && t < T_out && c < C) {
    const float* xp = x + (b * T_in + t / f) * C + c;
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(xp), x1 = *reinterpret_cast<const f32x4*>(xp + 4);
    float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    const int64_t orow = b * T_out + t;
    if (res) {
      float* rp = res + orow * C + c;
      *reinterpret_cast<f32x4*>(rp) = (f32x4){v[0] * res_mul, v[1] * res_mul, v[2] * res_mul, v[3] * res_mul};
      *reinterpret_cast<f32x4*>(rp + 4) = (f32x4){v[4] * res_mul, v[5] * res_mul, v[6] * res_mul, v[7] * res_mul};
    }
    if (film) {
      const float* fp = film + orow * ld_film + c;
      const f32x4 h0 = *reinterpret_cast<const f32x4*>(fp), h1 = *reinterpret_cast<const f32x4*>(fp + 4);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(fp + C), s1 = *reinterpret_cast<const f32x4*>(fp + C + 4);
      const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
      const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = fmaf(sc[i], v[i], sh[i]) * kWgInvSqrt2;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = v[i] >= 0.0f ? v[i] : slope * v[i];
    if (enc) {
      const float* ep = enc + b * ld_enc + c;
      const f32x4 e0 = *reinterpret_cast<const f32x4*>(ep), e1 = *reinterpret_cast<const f32x4*>(ep + 4);
      const float e[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += e[i];
    }
    o = (u32x4){pack2_bf16(v[0] * mul, v[1] * mul), pack2_bf16(v[2] * mul, v[3] * mul), pack2_bf16(v[4] * mul, v[5] * mul),
                pack2_bf16(v[6] * mul, v[7] * mul)};
  }
  if (out) *reinterpret_cast<u32x4*>(out + row * Cpad + c) = o;
}

__global__ __launch_bounds__(kWgThreads) void wg_last_conv_kernel(const float* __restrict__ x, int64_t T, int C, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, int taps, const float* audio_in,
                                                                  const float* __restrict__ noise, float c1, float c2, float sigma,
                                                                  float* audio_out, float* __restrict__ pred) {
  __shared__ float d[kWgMaxTaps][kWgLastRows + kWgMaxTaps - 1];
  const int64_t t0 = (int64_t)blockIdx.x * kWgLastRows, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = taps >> 1, nrows = kWgLastRows + taps - 1;
  for (int r = wave; r < nrows; r += kWgThreads / 64) {
    const int64_t tt = t0 + r - half;
    float acc[kWgMaxTaps];
#pragma unroll
    for (int j = 0; j < kWgMaxTaps; ++j) acc[j] = 0.0f;
    if (tt >= 0 && tt < T) {  // rows outside the utterance contribute zero
      const float* xr = x + (b * T + tt) * C;
      for (int c = lane * 4; c < C; c += 256) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
        for (int j = 0; j < kWgMaxTaps; ++j)
          if (j < taps) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (int64_t)j * C + c);
            acc[j] = fmaf(xv.w, wv.w, fmaf(xv.z, wv.z, fmaf(xv.y, wv.y, fmaf(xv.x, wv.x, acc[j]))));
          }
      }
    }
#pragma unroll
    for (int j = 0; j < kWgMaxTaps; ++j)
      if (j < taps) {
        const float s = wave_sum(acc[j]);
        if (lane == 0) d[j][r] = s;
      }
  }
  __syncthreads();
  const int64_t t = t0 + tid;
  if (tid < kWgLastRows && t < T) {
    float p = bias[0];
#pragma unroll
    for (int j = 0; j < kWgMaxTaps; ++j)
      if (j < taps) p += d[j][tid + j];  // out[t] reads row t + j - half with tap j: r = tid + j
    const int64_t o = b * T + t;
    if (pred) pred[o] = p;
    if (audio_out) {
      float v = c1 * (audio_in[o] - c2 * p);
      if (noise) v += sigma * noise[o];
      audio_out[o] = v;
    }
  }
}

static inline bool wg_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// ---- the plan: extents and checks ---------------------------------------------------------------------------------------------------
struct WgExtents {  // bytes each buffer of an op must hold (0: not used)
  int64_t in, in2, out, out2, residual;
};

// MA_OK and the extents, or the code ma_wavegrad_forward returns for this op.  No HIP call.
static int wg_op_extents(const ma_wavegrad_plan_t& pl, const ma_wavegrad_op_t& op, WgExtents& e) {
  e = WgExtents{0, 0, 0, 0, 0};
  const int64_t B = pl.B, T = op.T;
  if (T < 1 || (!op.w && op.kind != MA_WAVEGRAD_OP_PACK)) return MA_ERR_INVALID_ARG;
  switch (op.kind) {
    case MA_WAVEGRAD_OP_INIT:
      if (op.in != MA_WAVEGRAD_BUF_AUDIO || op.out < 0 || !op.bias || T != pl.T || op.N < 1) return MA_ERR_INVALID_ARG;
      e.out = B * T * op.N * 4;
      return MA_OK;
    case MA_WAVEGRAD_OP_PACK:
      if ((op.in < 0 && op.in != MA_WAVEGRAD_BUF_MEL) || (op.out < 0 && op.out2 < 0) || op.f < 1 || T % op.f || op.C < 1 || op.halo < 0)
        return MA_ERR_INVALID_ARG;
      if (op.in == MA_WAVEGRAD_BUF_MEL && (T / op.f != pl.frames || op.C != pl.n_mels)) return MA_ERR_INVALID_ARG;
      if (op.enc_off >= 0 && (op.enc_off + op.C > pl.enc_dim || (op.enc_off & 3))) return MA_ERR_INVALID_ARG;
      if (op.in2 >= 0 && op.ld_film < 2 * (int64_t)op.C) return MA_ERR_INVALID_ARG;
      if (op.in >= 0) e.in = B * (T / op.f) * op.C * 4;
      if (op.in2 >= 0) e.in2 = (B * T - 1) * op.ld_film * 4 + 2 * (int64_t)op.C * 4;
      if (op.out >= 0) e.out = B * (T + 2 * (int64_t)op.halo) * op.Cpad * 2;
      if (op.out2 >= 0) e.out2 = B * T * op.C * 4;
      return MA_OK;
    case MA_WAVEGRAD_OP_CONV:
      if (op.in < 0 || op.out < 0 || op.N < 1 || op.taps < 1 || !(op.taps & 1) || op.dilation < 1 || op.halo < 0 || op.Cpad < 1)
        return MA_ERR_INVALID_ARG;
      if (op.halo < (op.taps / 2) * op.dilation) return MA_ERR_INVALID_ARG;  // a tap would read the neighbouring utterance
      if (op.out_bf16 && (op.N & 63)) return MA_ERR_UNSUPPORTED;
      e.in = B * (T + 2 * (int64_t)op.halo) * op.Cpad * 2;
      e.out = B * T * op.N * (op.out_bf16 ? 2 : 4);
      if (op.residual >= 0) e.residual = B * T * op.N * 4;
      return MA_OK;
    case MA_WAVEGRAD_OP_DOWN:
      if (op.in < 0 || op.out < 0 || op.N < 1 || op.f < 1 || op.halo < 0 || op.Cpad < 1) return MA_ERR_INVALID_ARG;
      e.in = B * (T * op.f + 2 * (int64_t)op.halo) * op.Cpad * 2;
      e.out = B * T * op.N * 4;
      return MA_OK;
    case MA_WAVEGRAD_OP_LAST:
      if (op.in < 0 || !op.bias || T != pl.T || op.C < 1) return MA_ERR_INVALID_ARG;
      e.in = B * T * op.C * 4;
      return MA_OK;
    default:
      return MA_ERR_INVALID_ARG;
  }
}

// Bytes of workspace the plan reaches, or a negative code.  No HIP call.
static int64_t wg_plan_bytes(const ma_wavegrad_plan_t* pl) {
  if (!pl || !pl->ops || pl->n_ops < 1 || pl->B < 1 || pl->T < 1 || pl->frames < 1 || pl->n_mels < 1 || pl->enc_dim < 0 || (pl->enc_dim & 3))
    return MA_ERR_INVALID_ARG;
  if (pl->B > 65535) return MA_ERR_UNSUPPORTED;
  int64_t need = 0;
  bool last = false;
  for (int i = 0; i < pl->n_ops; ++i) {
    const ma_wavegrad_op_t& op = pl->ops[i];
    WgExtents e;
    const int rc = wg_op_extents(*pl, op, e);
    if (rc != MA_OK) return rc;
    const int64_t off[5] = {op.in, op.in2, op.out, op.out2, op.residual};
    const int64_t ext[5] = {e.in, e.in2, e.out, e.out2, e.residual};
    for (int k = 0; k < 5; ++k) {
      if (ext[k] == 0) continue;
      if (off[k] < 0 || (off[k] & 15)) return MA_ERR_INVALID_ARG;
      if (off[k] + ext[k] > need) need = off[k] + ext[k];
    }
    if (op.kind == MA_WAVEGRAD_OP_LAST) last = (i == pl->n_ops - 1);
  }
  return last ? need : MA_ERR_INVALID_ARG;  // the network ends in last_conv, and only there
}

struct WgStep {  // what changes from step to step
  const float* audio_in;
  const float* mel;
  const float* enc;
  int64_t ld_enc;
  const float* noise;
  float c1, c2, sigma;
  float* audio_out;
  float* pred;
};

static int wg_run_op(const ma_wavegrad_plan_t& pl, const ma_wavegrad_op_t& op, char* ws, const WgStep& st, ma_stream_t stream) {
  const int64_t B = pl.B, T = op.T;
  auto at = [&](int64_t off) -> char* { return off >= 0 ? ws + off : nullptr; };
  switch (op.kind) {
    case MA_WAVEGRAD_OP_INIT:
      return ma_wavegrad_init_conv_f32(st.audio_in, B, T, (const float*)op.w, op.bias, op.taps, op.N, (float*)at(op.out), stream);
    case MA_WAVEGRAD_OP_PACK: {
      const float* x = op.in == MA_WAVEGRAD_BUF_MEL ? st.mel : (const float*)at(op.in);
      return ma_wavegrad_pack_bf16(x, B, T / op.f, op.f, op.C, op.Cpad, op.halo, (const float*)at(op.in2), op.ld_film,
                                   op.enc_off >= 0 ? st.enc + op.enc_off : nullptr, st.ld_enc, op.slope, op.mul, at(op.out),
                                   (float*)at(op.out2), op.res_mul, stream);
    }
    case MA_WAVEGRAD_OP_CONV: {
      ma_gemm_epilogue_t e = {};
      e.bias = op.bias;
      e.alpha = op.alpha;
      e.out_bf16 = op.out_bf16;
      e.ldr = op.N;
      const int64_t rows_u = T + 2 * (int64_t)op.halo, osz = op.out_bf16 ? 2 : 4;
      for (int64_t b = 0; b < B; ++b) {
        e.residual = op.residual >= 0 ? (const float*)at(op.residual) + b * T * op.N : nullptr;
        const char* act = at(op.in) + (b * rows_u + op.halo) * op.Cpad * 2;  // the utterance's first real row
        const int rc = ma_conv1d_taps_bf16(act, op.Cpad, T, op.Cpad, op.taps, op.dilation, op.w, at(op.out) + b * T * op.N * osz, op.N,
                                           op.N, &e, stream);
        if (rc != MA_OK) return rc;
      }
      return MA_OK;
    }
    case MA_WAVEGRAD_OP_DOWN: {
      ma_gemm_epilogue_t e = {};
      e.bias = op.bias;
      e.alpha = op.alpha;
      const int64_t rows_u = T * op.f + 2 * (int64_t)op.halo, K = (int64_t)op.f * op.Cpad;
      for (int64_t b = 0; b < B; ++b) {
        const char* A = at(op.in) + (b * rows_u + op.halo) * op.Cpad * 2;
        const int rc = ma_gemm_bf16(A, K, op.w, K, at(op.out) + b * T * op.N * 4, op.N, T, op.N, K, &e, stream);
        if (rc != MA_OK) return rc;
      }
      return MA_OK;
    }
    default:  // MA_WAVEGRAD_OP_LAST (wg_plan_bytes has refused everything else)
      return ma_wavegrad_last_conv_update_f32((const float*)at(op.in), B, T, op.C, (const float*)op.w, op.bias, op.taps, st.audio_in,
                                              st.noise, st.c1, st.c2, st.sigma, st.audio_out, st.pred, stream);
  }
}

}  // namespace ma

using namespace ma;

extern "C" {

int ma_wavegrad_init_conv_f32(const float* audio, int64_t B, int64_t T, const float* wt, const float* bias, int32_t taps, int32_t C0,
                              float* out, ma_stream_t stream) {
  if (!audio || !wt || !bias || !out || B < 1 || T < 1 || C0 < 1 || taps < 1 || !(taps & 1)) return MA_ERR_INVALID_ARG;
  if (wg_misaligned(wt) || wg_misaligned(bias) || wg_misaligned(out)) return MA_ERR_INVALID_ARG;
  if (taps > kWgMaxTaps || (C0 & 3)) return MA_ERR_UNSUPPORTED;
  const int64_t total = B * T * (C0 >> 2), blocks = (total + kWgThreads - 1) / kWgThreads;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(wg_init_conv_kernel, dim3((unsigned)blocks), dim3(kWgThreads), 0, (hipStream_t)stream, audio, T, wt, bias, taps, C0, out, total);
  return MA_OK;
}

int ma_wavegrad_pack_bf16(const float* x, int64_t B, int64_t T_in, int32_t f, int32_t C, int32_t Cpad, int32_t halo, const float* film,
                          int64_t ld_film, const float* enc, int64_t ld_enc, float slope, float mul, void* out, float* res,
                          float res_mul, ma_stream_t stream) {
  if (!x || (!out && !res) || B < 1 || T_in < 1 || f < 1 || C < 1 || Cpad < C || halo < 0) return MA_ERR_INVALID_ARG;
  if (film && ld_film < 2 * (int64_t)C) return MA_ERR_INVALID_ARG;
  if (enc && ld_enc != 0 && ld_enc < C) return MA_ERR_INVALID_ARG;
  if (wg_misaligned(x) || wg_misaligned(film) || wg_misaligned(enc) || wg_misaligned(out) || wg_misaligned(res)) return MA_ERR_INVALID_ARG;
  if ((C & 7) || (Cpad & 63) || (film && (ld_film & 3)) || (enc && (ld_enc & 3))) return MA_ERR_UNSUPPORTED;
  const int64_t T_out = T_in * f;
  const int64_t total = B * (T_out + 2 * (int64_t)halo) * (Cpad >> 3), blocks = (total + kWgThreads - 1) / kWgThreads;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(wg_pack_kernel, dim3((unsigned)blocks), dim3(kWgThreads), 0, (hipStream_t)stream, x, T_in, T_out, f, C, Cpad, halo, film, ld_film,
            enc, ld_enc, slope, mul, reinterpret_cast<uint16_t*>(out), res, res_mul, total);
  return MA_OK;
}

int ma_wavegrad_last_conv_update_f32(const float* x, int64_t B, int64_t T, int32_t C, const float* w, const float* bias, int32_t taps,
                                     const float* audio_in, const float* noise, float c1, float c2, float sigma, float* audio_out,
                                     float* pred, ma_stream_t stream) {
  if (!x || !w || !bias || (!audio_out && !pred) || (audio_out && !audio_in) || B < 1 || T < 1 || C < 1 || taps < 1 || !(taps & 1))
    return MA_ERR_INVALID_ARG;
  if (wg_misaligned(x) || wg_misaligned(w)) return MA_ERR_INVALID_ARG;
  if (taps > kWgMaxTaps || (C & 3) || B > 65535) return MA_ERR_UNSUPPORTED;
  const int64_t blocks = (T + kWgLastRows - 1) / kWgLastRows;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(wg_last_conv_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(kWgThreads), 0, (hipStream_t)stream, x, T, C, w, bias, taps,
            audio_in, noise, c1, c2, sigma, audio_out, pred);
  return MA_OK;
}

int64_t ma_wavegrad_workspace_bytes(const ma_wavegrad_plan_t* plan) { return wg_plan_bytes(plan); }

int ma_wavegrad_forward(const ma_wavegrad_plan_t* plan, const float* audio, const float* mel, const float* enc, int64_t ld_enc,
                        float* pred, void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  const int64_t need = wg_plan_bytes(plan);
  if (need < 0) return (int)need;
  if (!audio || !mel || !pred || !workspace || (plan->enc_dim > 0 && !enc) || (ld_enc != 0 && ld_enc < plan->enc_dim) || (ld_enc & 3))
    return MA_ERR_INVALID_ARG;
  if (wg_misaligned(workspace) || wg_misaligned(mel) || wg_misaligned(enc)) return MA_ERR_INVALID_ARG;
  if (workspace_bytes < need) return MA_ERR_WORKSPACE;
  const WgStep st = {audio, mel, enc, ld_enc, nullptr, 0.0f, 0.0f, 0.0f, nullptr, pred};
  for (int i = 0; i < plan->n_ops; ++i) {
    const int rc = wg_run_op(*plan, plan->ops[i], static_cast<char*>(workspace), st, stream);
    if (rc != MA_OK) return rc;
  }
  return MA_OK;
}

int ma_wavegrad_reverse(const ma_wavegrad_plan_t* plan, float* audio, const float* mel, const float* enc_table, const float* c1,
                        const float* c2, const float* sigma, const float* noise, int32_t S, int32_t first_step, int32_t n_steps,
                        void* workspace, int64_t workspace_bytes, ma_stream_t stream) {
  const int64_t need = wg_plan_bytes(plan);
  if (need < 0) return (int)need;
  if (!audio || !mel || !c1 || !c2 || !sigma || !workspace || (plan->enc_dim > 0 && !enc_table) || S < 1 || first_step < 0 || n_steps < 1 ||
      (int64_t)first_step + n_steps > S)
    return MA_ERR_INVALID_ARG;
  // noise is needed by every iteration but the one with n == 0 (the last of the loop)
  if (!noise && !(n_steps == 1 && first_step == S - 1)) return MA_ERR_INVALID_ARG;
  if (wg_misaligned(workspace) || wg_misaligned(mel) || wg_misaligned(enc_table)) return MA_ERR_INVALID_ARG;
  if (workspace_bytes < need) return MA_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  WgStep st = {audio, mel, enc_table, 0, nullptr, 0.0f, 0.0f, 0.0f, audio, nullptr};
  for (int i = 0; i < plan->n_ops; ++i)
    if (plan->ops[i].once) {
      const int rc = wg_run_op(*plan, plan->ops[i], ws, st, stream);
      if (rc != MA_OK) return rc;
    }
  for (int32_t k = 0; k < n_steps; ++k) {
    const int32_t n = S - 1 - (first_step + k);
    st.enc = enc_table ? enc_table + (int64_t)n * plan->enc_dim : nullptr;
    st.noise = n > 0 ? noise + (int64_t)k * plan->B * plan->T : nullptr;
    st.c1 = c1[n];
    st.c2 = c2[n];
    st.sigma = sigma[n];
    for (int i = 0; i < plan->n_ops; ++i)
      if (!plan->ops[i].once) {
        const int rc = wg_run_op(*plan, plan->ops[i], ws, st, stream);
        if (rc != MA_OK) return rc;
      }
  }
  return MA_OK;
}

}  // extern "C"
