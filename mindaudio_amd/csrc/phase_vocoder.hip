// Phase vocoder of mindaudio/data/augment.py:828-871 (_phase_vocoder: time_stretch and pitch_shift stand on it).  Contract:
// include/mindaudio_amd.h.
//
// The reference walks the output frames in a Python loop and carries a phase accumulator, acc[t + 1] = acc[t] + inc[t] with
// inc[t] = phi + wrap(angle(c[i + 1]) - angle(c[i]) - phi), i = step_index[t].  inc[t] depends on the INPUT only, so the accumulator
// is a prefix sum: one workgroup per (row, 64-bin tile), lanes over bins, each of its kPvWaves waves owning a contiguous chunk of
// steps.  Pass 1 sums the chunk's increments per lane in float64, the chunk sums meet in LDS, every wave adds the sums of the waves
// before it in wave order, pass 2 walks its chunk again and emits.  No atomics; the order of every sum depends on T_out alone, a
// (row, bin) pair never meets another one: the same bits every run, and for a row alone or inside a batch.
//
// Angles, magnitudes, the mix and sine / cosine are float32; phi, the wrapped difference and the accumulator float64, reduced modulo
// 2 pi in float64 before the sine and cosine (the reference accumulates in the spectrogram's precision: DESIGN.md 8.2.1).
// Lanes over bins make frame-major reads (ma_stft_f32's MA_STFT_FRAME_MAJOR) coalesce; the bin-major output ma_istft_f32 reads is
// written through an LDS transpose, kPvTile steps of one bin side by side.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kPvWaves = 8;  // waves per workgroup = chunks of the scan
constexpr int kPvTile = 8;   // steps a wave emits between two transposes: 64-byte runs per bin in `out`
constexpr double kPvTwoPi = 6.283185307179586476925286766559;
constexpr double kPvInvTwoPi = 0.15915494309189533576888376337251;

// one (row, bin) of the spectrogram: column j lives at base[j * stride]; columns outside [0, frames) are the reference's zero padding
// (angle 0, magnitude 0) and are never read
struct PvColumn {
  const float2* base;
  int64_t stride;
  int frames;
  bool live;  // the lane's bin exists
};

template <bool kMag>
__device__ __forceinline__ void pv_read(const PvColumn& col, int j, float& ang, float& mag) {
  float2 c = make_float2(0.0f, 0.0f);
  if (col.live && (unsigned)j < (unsigned)col.frames) c = col.base[(int64_t)j * col.stride];
  ang = atan2f(c.y, c.x);
  if (kMag) mag = hypotf(c.x, c.y);
}

// The pair of columns (i, i + 1) of a step.  Consecutive steps mostly share columns (rate < 1: the same pair; rate <= 2: the second
// becomes the first), `i` is the same in every lane, so the branches are uniform and what is reused is the same value it would have
// been computed to.
template <bool kMag>
struct PvPair {
  int cur = INT32_MIN / 2;
  float a0 = 0.0f, m0 = 0.0f, a1 = 0.0f, m1 = 0.0f;
  __device__ __forceinline__ void seek(const PvColumn& col, int i) {
    if (i == cur) return;
    if (i == cur + 1) {
      a0 = a1;
      m0 = m1;
    } else {
      pv_read<kMag>(col, i, a0, m0);
    }
    pv_read<kMag>(col, i + 1, a1, m1);
    cur = i;
  }
  // phi + (d - 2 pi round(d / 2 pi)), d = angle(c1) - angle(c0) - phi
  __device__ __forceinline__ double increment(double phi) const {
    double d = (double)a1 - (double)a0 - phi;
    d -= kPvTwoPi * rint(d * kPvInvTwoPi);
    return phi + d;
  }
};

__global__ __launch_bounds__(kPvWaves * 64) void phase_vocoder_kernel(const float2* __restrict__ spec, int bin_major, int frames,
                                                                      int n_freq, const int32_t* __restrict__ step_index,
                                                                      const double* __restrict__ step_alpha, int t_out, double phi_step,
                                                                      double phi_last, int tiles, float2* __restrict__ out) {
  __shared__ double chunk_sum[kPvWaves][64];
  __shared__ float2 tile[kPvWaves][64][kPvTile + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = blockIdx.x / tiles;
  const int k0 = (int)(blockIdx.x % tiles) * 64, k = k0 + lane;
  PvColumn col;
  col.live = k < n_freq;
  col.frames = frames;
  col.stride = bin_major ? 1 : n_freq;
  col.base = spec + row * (int64_t)frames * n_freq + (col.live ? (bin_major ? (int64_t)k * frames : (int64_t)k) : 0);
  const double phi = k == n_freq - 1 ? phi_last : (double)k * phi_step;  // np.linspace(0, pi hop, n_freq)[k]
  // every wave walks chunk / kPvTile sub-tiles (the barriers below are uniform); its steps are [t_lo, t_hi)
  const int chunk = (t_out + kPvWaves * kPvTile - 1) / (kPvWaves * kPvTile) * kPvTile;
  const int t_lo = min(w * chunk, t_out), t_hi = min(t_lo + chunk, t_out);

  {  // pass 1: the chunk's increments, summed in step order
    PvPair<false> p;
    double sum = 0.0;
    for (int t = t_lo; t < t_hi; ++t) {
      p.seek(col, step_index[t]);
      sum += p.increment(phi);
    }
    chunk_sum[w][lane] = sum;
  }
  __syncthreads();
  double acc;
  {
    float a, m;
    pv_read<false>(col, 0, a, m);
    acc = (double)a;  // acc[0] = angle(column 0)
    for (int v = 0; v < w; ++v) acc += chunk_sum[v][lane];
  }

  PvPair<true> p;
  float2* orow = out + (row * n_freq + k0) * (int64_t)t_out;
  for (int s0 = 0; s0 < chunk; s0 += kPvTile) {
    const int t0 = t_lo + s0;
#pragma unroll
    for (int s = 0; s < kPvTile; ++s) {
      const int t = t0 + s;
      if (t < t_hi) {
        p.seek(col, step_index[t]);
        const float alpha = (float)step_alpha[t];
        const float mag = (1.0f - alpha) * p.m0 + alpha * p.m1;
        const float r = (float)(acc - kPvTwoPi * rint(acc * kPvInvTwoPi));
        float sn, cs;
        sincosf(r, &sn, &cs);
        tile[w][lane][s] = make_float2(mag * cs, mag * sn);
        acc += p.increment(phi);
      }
    }
    __syncthreads();
    // lane -> (bin, step): kPvTile consecutive steps of one bin are one contiguous run of `out`
#pragma unroll
    for (int e = lane; e < 64 * kPvTile; e += 64) {
      const int bin = e / kPvTile, s = e % kPvTile;
      if (t0 + s < t_hi && k0 + bin < n_freq) orow[(int64_t)bin * t_out + t0 + s] = tile[w][bin][s];
    }
    __syncthreads();
  }
}

}  // namespace ma

using namespace ma;

extern "C" int ma_phase_vocoder_f32(const float* spec, int32_t in_layout, int64_t B, int64_t frames, int32_t n_freq,
                                    const int32_t* step_index, const double* step_alpha, int64_t T_out, int32_t hop, float* out,
                                    ma_stream_t stream) {
  if (hop < 1) return MA_ERR_HOP;
  if (!spec || !step_index || !step_alpha || !out || B < 1 || frames < 1 || n_freq < 2 || T_out < 1 ||
      (in_layout != MA_STFT_FRAME_MAJOR && in_layout != MA_STFT_FREQ_MAJOR))
    return MA_ERR_INVALID_ARG;
  const int64_t tiles = ((int64_t)n_freq + 63) / 64;
  if (frames > 0x3fffffff || T_out > 0x3fffffff || B * tiles > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  const double phi_last = M_PI * (double)hop;
  MA_LAUNCH(phase_vocoder_kernel, dim3((unsigned)(B * tiles)), dim3(kPvWaves * 64), 0, (hipStream_t)stream,
            reinterpret_cast<const float2*>(spec), (int)(in_layout == MA_STFT_FREQ_MAJOR), (int)frames, (int)n_freq, step_index,
            step_alpha, (int)T_out, phi_last / (double)(n_freq - 1), phi_last, (int)tiles, reinterpret_cast<float2*>(out));
  return MA_OK;
}
