// Layer-pipelined unidirectional LSTM stack, inference (mindaudio/models/tasnet.py Separator: nn.LSTM(N, hidden, num_layers,
// bidirectional=False)).  Contract: include/mindaudio_amd.h.  The tile, the cell, the packed weights' fragment order and the K loop
// are lstm_common.h's; this file holds the schedule, the state's parity argument and the two ways a workgroup covers its batch rows.
//
// Schedule.  Layer l at time t needs layer l - 1 at time t and itself at t - 1, so every (l, t) with t + l = d can run at once.  The host
// loop of ma_lstm_stack_bf16 walks the diagonals d = 0 .. T + n_layers - 2 and issues ONE LAUNCH PER DIAGONAL; blockIdx.y spans the
// layers that are active on it, max(0, d - T + 1) .. min(n_layers - 1, d), and layer l computes t = d - l.  The stream order between
// those launches is the only synchronisation: no workgroup ever waits for another one (no grid barrier, no flags, no cooperative
// launch, no atomics, no graph capture).
//
// Cell.  gates (B, 4H) = [x_t | h_{t-1}] . [W_ih | W_hh]^T + (b_ih + b_hh) in ONE K loop over K = Kin + H (Kin = Kpad for layer 0, H
// above it): there is no projection GEMM and no projection buffer.  The weights are packed once per layer (ma_lstm_stack_pack_f32).
// The A operand of layer 0 is x[t], that of layer l >= 1 the bf16 h image of layer l - 1; the recurrent half of K reads the layer's
// own h image.  Two forms:
//   lstm_stack_ksplit_kernel (B <= 16, one batch tile): the four waves split the k-steps between them (32 at H = Kpad = 512: 8 each,
//     all in flight at once), leave their partial gate sums in LDS (16 KB) and meet at one workgroup barrier; then wave w sums the four
//     partials IN WAVE ORDER for register index w (batch rows 4 (lane >> 4) + w) and runs that quarter of the cell.
//   lstm_stack_tile_kernel (B > 16): grid.z = ceil(B / 64), wave w runs all of K for batch rows 64 z + 16 w .. + 15; no LDS, no barrier.
//
// State and the parity argument.  Per layer: TWO (B, H) bf16 images of h and one (B, H) float32 c.
//   (1) every write of h on diagonal d goes to image d & 1 of the writing layer;
//   (2) every read of h on diagonal d comes from image (d - 1) & 1: the layer's own h_{t-1} was written by (l, t - 1), which lies on
//       diagonal d - 1, and the lower layer's h_t was written by (l - 1, t), which lies on diagonal d - 1 as well;
//   (3) so the images a launch reads and the images it writes are disjoint, whichever layers share it, and what it reads was
//       completed by the PREVIOUS launch, which the stream order puts before it;
//   (4) image (d - 1) & 1 is not written again before diagonal d + 1, i.e. after this launch has finished;
//   (5) layer l first runs on diagonal d = l (t = 0) and reads its own image (l - 1) & 1, which it has never written (its first write
//       goes to image l & 1): both images are zeroed once before the loop, hence h_0 = 0 for every layer;
//   (6) c[l] is read and written by layer l alone, each element by ONE lane of one workgroup per launch (loaded before the K loop,
//       stored after the cell), and zeroed once: c_0 = 0.
// Only the last layer writes out_f32 / out_bf16; the layers below write nothing but their h image and c.  h_final / c_final are stored
// by the cell of t = T - 1 of each layer.
//
// Rounding points (those of a layer-by-layer run): x, the weights and every h that feeds a product are bf16 (round to nearest even);
// gate sums, c, the output and h_final are float32; accumulation is float32 in a fixed order, so two runs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "launch.h"
#include "lstm_common.h"

namespace ma {

constexpr int kStackMaxLayers = 8;

struct StackStep {
  const uint16_t* w[kStackMaxLayers];  // packed [W_ih | W_hh] per layer
  const float* bias[kStackMaxLayers];  // (4H) per layer
  const uint16_t* x;                   // (T, B, Kpad) bf16
  uint16_t* h;                         // (n_layers, 2, B, H) bf16 images
  float* c;                            // (n_layers, B, H)
  float* out_f32;                      // (T, B, H)
  uint16_t* out_bf16;                  // (T, B, H) or null
  float* h_final;                      // (n_layers, B, H) or null
  float* c_final;
  int64_t T, d;
  int32_t l0, n_layers, B, H, Kpad;
};

// where layer l on diagonal d finds its operands and leaves its state
struct StackLayer {
  const uint16_t* in;     // row 0 of the input half of A: x[t] (layer 0) or the lower layer's h image (d - 1) & 1
  const uint16_t* h_prev;  // the layer's own image (d - 1) & 1
  uint16_t* h_next;        // the layer's own image d & 1
  const uint16_t* w;
  const float* bias;
  float* c;
  int64_t t;
  int l, ld_in, nk_in, nk;
};
__device__ __forceinline__ StackLayer stack_layer(const StackStep& p) {
  StackLayer s;
  const int l = p.l0 + (int)blockIdx.y;
  const int64_t bh = (int64_t)p.B * p.H;
  const int rd = (int)((p.d + 1) & 1), wr = (int)(p.d & 1);  // (d - 1) & 1 == (d + 1) & 1
  s.l = l;
  s.t = p.d - l;
  s.ld_in = l == 0 ? p.Kpad : p.H;
  s.in = l == 0 ? p.x + s.t * p.B * (int64_t)p.Kpad : p.h + ((int64_t)(l - 1) * 2 + rd) * bh;
  s.h_prev = p.h + ((int64_t)l * 2 + rd) * bh;
  s.h_next = p.h + ((int64_t)l * 2 + wr) * bh;
  s.w = p.w[l];
  s.bias = p.bias[l];
  s.c = p.c + (int64_t)l * bh;
  s.nk_in = s.ld_in / 32;
  s.nk = s.nk_in + p.H / 32;
  return s;
}

// The A operand of one batch tile: k-steps below nk_in come from the layer's input, the rest from its own h image.
struct StackA {
  const uint16_t *in, *h;  // this lane's row (rows beyond B take row 0's) at the lane's column of k-step 0 of each half;
  int nk_in;               // `h` is biased by the input half's width, so that both halves are addressed by the k-step index alone
  __device__ __forceinline__ StackA(const StackStep& p, const StackLayer& s, int b0, int lane) : nk_in(s.nk_in) {
    const int arow = b0 + (lane & 15) < p.B ? b0 + (lane & 15) : 0;
    in = s.in + (int64_t)arow * s.ld_in + 8 * (lane >> 4);
    h = s.h_prev + (int64_t)arow * p.H + 8 * (lane >> 4) - (int64_t)s.nk_in * 32;
  }
  __device__ __forceinline__ const uint16_t* operator()(int, int kk) const { return (kk < nk_in ? in : h) + kk * 32; }
};

// The cell of one (batch row b, hidden unit j) and where its state and outputs go.  Lane-local.
__device__ __forceinline__ void stack_cell(const StackStep& p, const StackLayer& s, int b, int j, float gi, float gf, float gg, float go,
                                           float c_prev) {
  const int64_t e = (int64_t)b * p.H + j;
  const LstmCell n = lstm_cell(gi, gf, gg, go, c_prev);
  s.c[e] = n.c;
  s.h_next[e] = f2bf(n.h);
  if (s.l == p.n_layers - 1) {
    const int64_t o = s.t * p.B * (int64_t)p.H + e;
    p.out_f32[o] = n.h;
    if (p.out_bf16) p.out_bf16[o] = f2bf(n.h);
  }
  if (s.t == p.T - 1) {
    const int64_t o = (int64_t)s.l * p.B * p.H + e;
    if (p.h_final) p.h_final[o] = n.h;
    if (p.c_final) p.c_final[o] = n.c;
  }
}

// B <= 16.  KB = k-steps per operand block; the launcher picks it so that every wave's share nk / 4 is a multiple of KB (KB = 1 also
// serves an nk that is no multiple of 4: the shares are then [w nk / 4, (w + 1) nk / 4), each at least one k-step since nk >= 4).
template <int KB>
__global__ __launch_bounds__(kLstmThreads) void lstm_stack_ksplit_kernel(const StackStep p) {
  __shared__ float part[4 * 16 * 64];  // [source wave][gate * 4 + register][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const StackLayer s = stack_layer(p);
  const int H = p.H, sl = blockIdx.x;
  // this thread's quarter of the cell: register index `wave` of the C/D map
  const int b = 4 * (lane >> 4) + wave, j = sl * kLstmSlice + (lane & 15);
  const bool ok = b < p.B;
  f32x4 acc[1][4];
  float bias[4], c_prev;
  lstm_k_loop<KB>(lstm_gate_run(s.w, s.nk, sl, 0, lane), StackA(p, s, 0, lane), wave * s.nk / 4, (wave + 1) * s.nk / 4, acc, [&] {
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = s.bias[g * H + j];
    c_prev = ok ? s.c[(int64_t)b * H + j] : 0.0f;
  });

  float* dst = part + (wave * 16) * 64 + lane;
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(g * 4 + r) * 64] = acc[0][g][r];
  __syncthreads();  // (within the workgroup; every wave arrives: nothing returns before this line)
  float gate[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float v = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) v += part[((w * 16) + g * 4 + wave) * 64 + lane];  // wave order = K order
    gate[g] = v + bias[g];
  }
  if (ok) stack_cell(p, s, b, j, gate[0], gate[1], gate[2], gate[3], c_prev);
}

// B > 16: each wave runs all of K for its own 16 batch rows (nk is even: blocks of 2 k-steps).
__global__ __launch_bounds__(kLstmThreads) void lstm_stack_tile_kernel(const StackStep p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b0 = ((int)blockIdx.z * 4 + wave) * 16;
  if (b0 >= p.B) return;  // (no barrier anywhere in this kernel)
  const StackLayer s = stack_layer(p);
  const int H = p.H, sl = blockIdx.x;
  const int j = sl * kLstmSlice + (lane & 15);
  f32x4 acc[1][4];
  float bias[4], c_prev[4];
  lstm_k_loop<2>(lstm_gate_run(s.w, s.nk, sl, 0, lane), StackA(p, s, b0, lane), 0, s.nk, acc, [&] {
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = s.bias[g * H + j];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + 4 * (lane >> 4) + r;
      c_prev[r] = b < p.B ? s.c[(int64_t)b * H + j] : 0.0f;
    }
  });
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + 4 * (lane >> 4) + r;
    if (b < p.B)
      stack_cell(p, s, b, j, acc[0][0][r] + bias[0], acc[0][1][r] + bias[1], acc[0][2][r] + bias[2], acc[0][3][r] + bias[3], c_prev[r]);
  }
}

// [W_ih | W_hh] of one layer -> fragment order; columns K .. Kpad - 1 of the W_ih half are zero; bias = b_ih + b_hh
__global__ __launch_bounds__(256) void lstm_stack_pack_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                                              const float* __restrict__ b_ih, const float* __restrict__ b_hh, int K, int Kpad,
                                                              int H, int64_t groups, uint16_t* __restrict__ out, float* __restrict__ bias) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one 8-element fragment
  if (i < 4 * (int64_t)H) bias[i] = b_ih[i] + b_hh[i];
  if (i >= groups) return;
  const LstmFragment f = lstm_fragment(i, (Kpad + H) / 32);
  const int64_t row = (int64_t)f.gate * H + f.unit;
  if (f.k < Kpad) lstm_pack_fragment(w_ih + row * K, f.k, K, out + i * 8);
  else lstm_pack_fragment(w_hh + row * H, f.k - Kpad, H, out + i * 8);
}

struct StackWs {
  int64_t h, c, total;  // byte offsets
};
static StackWs stack_ws(int64_t B, int64_t H, int64_t n_layers) {
  StackWs w;
  w.h = 0;
  w.c = w.h + align256(n_layers * 2 * B * H * 2);
  w.total = w.c + align256(n_layers * B * H * 4);
  return w;
}

static bool stack_shape_ok(int64_t T, int64_t B, int64_t Kpad, int64_t H, int64_t n_layers) {
  return lstm_shape_ok(T, B, Kpad, H) && n_layers >= 1 && n_layers <= kStackMaxLayers && Kpad <= 0x3fffffff;
}

}  // namespace ma

using namespace ma;

extern "C" {

int64_t ma_lstm_stack_workspace_bytes(int64_t T, int64_t B, int32_t H, int32_t n_layers) {
  if (T < 1 || B < 1 || H < 1 || n_layers < 1) return MA_ERR_INVALID_ARG;
  if (!stack_shape_ok(T, B, 64, H, n_layers)) return MA_ERR_UNSUPPORTED;
  return stack_ws(B, H, n_layers).total;
}

int ma_lstm_stack_pack_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int32_t K, int32_t Kpad, int32_t H,
                           void* packed, float* bias, ma_stream_t stream) {
  if (!w_ih || !w_hh || !b_ih || !b_hh || !packed || !bias || K < 1 || Kpad < K || H < 1) return MA_ERR_INVALID_ARG;
  if (!stack_shape_ok(1, 1, Kpad, H, 1)) return MA_ERR_UNSUPPORTED;
  if (!lstm_aligned16(packed, bias)) return MA_ERR_INVALID_ARG;
  const int64_t groups = 4 * (int64_t)H * (Kpad + H) / 8;
  MA_LAUNCH(lstm_stack_pack_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_ih, w_hh, b_ih, b_hh, K,
            Kpad, H, groups, reinterpret_cast<uint16_t*>(packed), bias);
  return MA_OK;
}

int ma_lstm_stack_bf16(const void* x, int64_t T, int64_t B, int32_t Kpad, int32_t H, int32_t n_layers, const void* const* packed,
                       const float* const* bias, float* out_f32, void* out_bf16, float* h_final, float* c_final, void* workspace,
                       int64_t workspace_bytes, ma_stream_t stream) {
  if (!x || !packed || !bias || !out_f32 || !workspace || T < 1 || B < 1 || Kpad < 1 || H < 1 || n_layers < 1) return MA_ERR_INVALID_ARG;
  if (!stack_shape_ok(T, B, Kpad, H, n_layers)) return MA_ERR_UNSUPPORTED;
  for (int l = 0; l < n_layers; ++l)
    if (!packed[l] || !bias[l] || !lstm_aligned16(packed[l], bias[l])) return MA_ERR_INVALID_ARG;
  if (!lstm_aligned16(x, workspace)) return MA_ERR_INVALID_ARG;
  const StackWs ws = stack_ws(B, H, n_layers);
  if (workspace_bytes < ws.total) return MA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(workspace);
  if (ensure_init() != MA_OK) return MA_ERR_LAUNCH;

  StackStep p;
  for (int l = 0; l < kStackMaxLayers; ++l) {
    p.w[l] = l < n_layers ? reinterpret_cast<const uint16_t*>(packed[l]) : nullptr;
    p.bias[l] = l < n_layers ? bias[l] : nullptr;
  }
  p.x = reinterpret_cast<const uint16_t*>(x);
  p.h = reinterpret_cast<uint16_t*>(base + ws.h);
  p.c = reinterpret_cast<float*>(base + ws.c);
  p.out_f32 = out_f32;
  p.out_bf16 = reinterpret_cast<uint16_t*>(out_bf16);
  p.h_final = h_final;
  p.c_final = c_final;
  p.T = T;
  p.n_layers = n_layers;
  p.B = (int32_t)B;
  p.H = H;
  p.Kpad = Kpad;
  // h_0 = c_0 = 0 for every layer: BOTH h images (point 5 of the parity argument)
  if (hipMemsetAsync(p.h, 0, (size_t)(n_layers * 2 * B * H * 2), st) != hipSuccess) return MA_ERR_LAUNCH;
  if (hipMemsetAsync(p.c, 0, (size_t)(n_layers * B * H * 4), st) != hipSuccess) return MA_ERR_LAUNCH;

  const bool small = B <= 16;
  // the k-steps of a layer: layer 0 has (Kpad + H) / 32, the others 2 H / 32; the ksplit block size must suit every active layer
  const int nk0 = (Kpad + H) / 32, nk1 = 2 * H / 32;
  auto block_of = [](int nk) { return nk % 32 == 0 ? 8 : nk % 16 == 0 ? 4 : nk % 8 == 0 ? 2 : 1; };
  const int kb_all = n_layers > 1 ? (block_of(nk0) < block_of(nk1) ? block_of(nk0) : block_of(nk1)) : block_of(nk0);
  const int kb_upper = block_of(nk1);
  const unsigned gz = small ? 1u : (unsigned)((B + kLstmRowsPerWg - 1) / kLstmRowsPerWg);
  for (int64_t d = 0; d < T + n_layers - 1; ++d) {
    const int l0 = (int)(d - T + 1 > 0 ? d - T + 1 : 0), l1 = (int)(d < n_layers - 1 ? d : n_layers - 1);
    p.d = d;
    p.l0 = l0;
    const dim3 grid((unsigned)(H / kLstmSlice), (unsigned)(l1 - l0 + 1), gz);
    if (!small) {
      MA_LAUNCH(lstm_stack_tile_kernel, grid, dim3(kLstmThreads), 0, st, p);
      continue;
    }
    const int kb = l0 == 0 ? kb_all : kb_upper;
    if (kb == 8) MA_LAUNCH(lstm_stack_ksplit_kernel<8>, grid, dim3(kLstmThreads), 0, st, p);
    else if (kb == 4) MA_LAUNCH(lstm_stack_ksplit_kernel<4>, grid, dim3(kLstmThreads), 0, st, p);
    else if (kb == 2) MA_LAUNCH(lstm_stack_ksplit_kernel<2>, grid, dim3(kLstmThreads), 0, st, p);
    else MA_LAUNCH(lstm_stack_ksplit_kernel<1>, grid, dim3(kLstmThreads), 0, st, p);
  }
  return MA_OK;
}

}  // extern "C"
