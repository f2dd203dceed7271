// DeepSpeech2 (mindaudio/models/deepspeech2.py) outside its LSTM stack (lstm.hip) and its GEMMs: the first convolution of MaskConv
// and the softmax + transpose of PredictWithSoftmax.  Contract: include/mindaudio_amd.h.
//
// conv1 = Conv2d(1 -> 32, (41, 11), stride (2, 2), pad (20, 5)) + BatchNorm2d (inference, folded by the caller into a per-channel
// scale and shift) + tanh: one input channel and 451 taps, so it is a direct float32 kernel (a tenth of the front end's FLOPs).  Its
// output is the activation layout of the second convolution, which runs on MFMA as ma_conv1d_taps_bf16 over TIME:
//   (T1 + 10 frames, B, Fpad, 32) bf16, time-major, channel-last, frequency rows 10 .. 10 + F1 - 1 hold the values, the rows around
//   them and the 5 frames before and after stay zero (the caller zeroes the buffer once; only the interior is ever written).
// With the rows ordered (frame, utterance) a dilation of B rows is one frame of the same utterance, the 21 frequency taps x 32
// channels of an output frequency are one contiguous run of the row, and the output rows are already the (T1, B, features) input
// of the LSTM stack.
//
// A workgroup holds the transposed weights (451, 32) and one frame's input patch ((F + 40) x 11, zero padded) in LDS; thread
// (cq = tid & 7, g = tid >> 3) owns the four channels 4 cq .. 4 cq + 3 of the output frequencies g, g + 32, ...: per tap one 16-byte
// LDS read of its four weights and one 4-byte read per output frequency feed 4 FMAs each (a thread that owns ONE channel reads one
// LDS word per FMA and is bound by the LDS: 84.6 ms for this launch at the yaml evaluation shape).  A wave's eight frequencies are 22 words apart
// (banks 0, 22, 12, 2, 24, 14, 4, 26: no conflict), its eight channel quads are 128 contiguous bytes.
// Accumulation: a float32 fmaf chain over the taps in (frequency tap, time tap) order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kDsC = 32, kDsKf = 41, kDsKt = 11, kDsTaps = kDsKf * kDsKt;
constexpr int kDsMaxF = 256;        // F1 <= 128 = 32 frequency groups x kDsNi outputs per thread
constexpr int kDsNi = 4;
constexpr int kDsFramesPerWg = 8;
constexpr int kDsLds = kDsTaps * kDsC * 4 + (kDsMaxF + 40) * kDsKt * 4;

__global__ __launch_bounds__(256) void ds2_conv1_kernel(const float* __restrict__ x, int F, int T, int B, int F1, int T1,
                                                        const float* __restrict__ wt, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, int Fpad, uint16_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = reinterpret_cast<float*>(smem);  // (451, 32)
  float* patch = wl + kDsTaps * kDsC;          // (F + 40, 11): input rows f - 20, columns 2 t1 - 5 + kt
  const int tid = threadIdx.x, cq = tid & 7, g = tid >> 3;  // channels 4 cq .. 4 cq + 3, output frequencies g, g + 32, ...
  const int b = blockIdx.y;
  for (int i = tid; i < kDsTaps * kDsC; i += 256) wl[i] = wt[i];
  const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + 4 * cq), sh = *reinterpret_cast<const f32x4*>(shift + 4 * cq);
  const int prow = F + 40;
  const float* xb = x + (int64_t)b * F * T;
  for (int it = 0; it < kDsFramesPerWg; ++it) {
    const int t1 = blockIdx.x * kDsFramesPerWg + it;
    if (t1 >= T1) break;  // (uniform over the workgroup)
    __syncthreads();      // the previous frame's patch has been read; (first pass) nothing
    for (int i = tid; i < prow * kDsKt; i += 256) {
      const int r = i / kDsKt, kt = i - r * kDsKt;
      const int f = r - 20, t = 2 * t1 - 5 + kt;
      patch[i] = (f >= 0 && f < F && t >= 0 && t < T) ? xb[(int64_t)f * T + t] : 0.0f;
    }
    __syncthreads();
    f32x4 acc[kDsNi];
#pragma unroll
    for (int i = 0; i < kDsNi; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kf = 0; kf < kDsKf; ++kf)
      for (int kt = 0; kt < kDsKt; ++kt) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wl + (kf * kDsKt + kt) * kDsC + 4 * cq);
#pragma unroll
        for (int i = 0; i < kDsNi; ++i) {
          const int f1 = g + 32 * i;
          if (f1 < F1) {
            const float xv = patch[(2 * f1 + kf) * kDsKt + kt];  // row 2 f1 + kf <= F - 1 + 40
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(w[c], xv, acc[i][c]);
          }
        }
      }
    uint16_t* o = out + (((int64_t)(t1 + 5) * B + b) * Fpad + 10) * kDsC + 4 * cq;
#pragma unroll
    for (int i = 0; i < kDsNi; ++i) {
      const int f1 = g + 32 * i;
      if (f1 < F1) {
        float y[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = tanhf(fmaf(acc[i][c], sc[c], sh[c]));
        uint2 v;
        v.x = (uint32_t)f2bf(y[0]) | ((uint32_t)f2bf(y[1]) << 16);
        v.y = (uint32_t)f2bf(y[2]) | ((uint32_t)f2bf(y[3]) << 16);
        *reinterpret_cast<uint2*>(o + (int64_t)f1 * kDsC) = v;  // 8-byte aligned: 4 cq channels of a 32-channel row
      }
    }
  }
}
MA_LDS_ATTR(ds2_conv1_kernel, kDsLds);

// probs[b, t, :] = softmax(logits[t, b, :C]); one wave per (t, b) row
__global__ __launch_bounds__(256) void ds2_softmax_kernel(const float* __restrict__ logits, int64_t ld, int64_t T, int64_t B, int C,
                                                          float* __restrict__ probs) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // = t * B + b
  if (row >= T * B) return;
  const int lane = threadIdx.x & 63;
  const float* in = logits + row * ld;
  const int64_t t = row / B, b = row - t * B;
  float* o = probs + (b * T + t) * C;
  float m = -INFINITY;
  for (int i = lane; i < C; i += 64) m = fmaxf(m, in[i]);
  m = wave_max(m);
  float s = 0.0f;
  for (int i = lane; i < C; i += 64) s += expf(in[i] - m);
  s = wave_sum(s);
  for (int i = lane; i < C; i += 64) o[i] = expf(in[i] - m) / s;
}

}  // namespace ma

using namespace ma;

extern "C" {

int ma_ds2_conv1_bf16(const float* x, int64_t B, int32_t F, int64_t T, const float* wt, const float* scale, const float* shift,
                      int32_t Fpad, void* out, ma_stream_t stream) {
  if (!x || !wt || !scale || !shift || !out || B < 1 || F < 1 || T < 1) return MA_ERR_INVALID_ARG;
  const int F1 = (F - 1) / 2 + 1;
  const int64_t T1 = (T - 1) / 2 + 1;
  if (F > kDsMaxF || B > 65535 || T1 > 0x7fffffff / 2 || Fpad < F1 + 20) return MA_ERR_UNSUPPORTED;
  const int lds = kDsTaps * kDsC * 4 + (F + 40) * kDsKt * 4;
  MA_LAUNCH(ds2_conv1_kernel, dim3((unsigned)((T1 + kDsFramesPerWg - 1) / kDsFramesPerWg), (unsigned)B), dim3(256), lds,
            (hipStream_t)stream, x, F, (int)T, (int)B, F1, (int)T1, wt, scale, shift, Fpad, reinterpret_cast<uint16_t*>(out));
  return MA_OK;
}

int ma_ds2_softmax_f32(const float* logits, int64_t ld, int64_t T, int64_t B, int32_t C, float* probs, ma_stream_t stream) {
  if (!logits || !probs || T < 1 || B < 1 || C < 1 || ld < C) return MA_ERR_INVALID_ARG;
  if ((T * B + 3) / 4 > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(ds2_softmax_kernel, dim3((unsigned)((T * B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, ld, T, B, C, probs);
  return MA_OK;
}

}  // extern "C"
