// What the Conv-TasNet kernel files share (conv_tasnet.hip: inference, conv_tasnet_train.hip: training): the tile geometry, the
// workgroup sums, the float64 moments that global layer norm travels as, and the launchers' shape checks.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"

namespace ma {

constexpr int kTnThreads = 256;
constexpr int kTnTileElems = 8192;  // values of a tile at most: 32 per thread
constexpr int kTnIter4 = kTnTileElems / 4 / kTnThreads;
constexpr double kGlnEps = 1e-8;

static int tile_rows(int C) { return kTnTileElems / C; }  // (C <= kTnTileElems: check_tiles)

// sum over the workgroup's 4 waves, waves added in index order; every thread gets the result
__device__ __forceinline__ double tile_sum(double v, double* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return r;
}

// the tile's (count, sum, centred second moment) from per-thread sums; `centred(mean)` returns the thread's sum of (v - mean)^2
template <class F>
__device__ __forceinline__ void tile_moments(double thread_sum, int64_t count, double* sh, double* part, F&& centred) {
  const double s = tile_sum(thread_sum, sh);
  const double mean = s / (double)count;
  const double m2 = tile_sum(centred(mean), sh);
  if (threadIdx.x == 0) {
    part[0] = (double)count;
    part[1] = s;
    part[2] = m2;
  }
}

// mean and 1 / sqrt(var + eps) of an utterance from its partials (wave 0 joins them, lane p takes partials p, p + 64, ...)
__device__ __forceinline__ void gln_mean_rstd_f64(const double* __restrict__ part, int nparts, double* sh, double& mean, double& rstd) {
  if (threadIdx.x < 64) {
    double n = 0.0, s = 0.0;
    for (int p = threadIdx.x; p < nparts; p += 64) {
      n += part[3 * p];
      s += part[3 * p + 1];
    }
    n = wave_sum(n);
    s = wave_sum(s);
    const double mu = s / n;
    double m2 = 0.0;
    for (int p = threadIdx.x; p < nparts; p += 64) {
      const double np = part[3 * p], d = part[3 * p + 1] / np - mu;
      m2 += part[3 * p + 2] + np * d * d;
    }
    m2 = wave_sum(m2);
    if (threadIdx.x == 0) {
      sh[0] = mu;
      sh[1] = 1.0 / sqrt(m2 / n + kGlnEps);
    }
  }
  __syncthreads();
  mean = sh[0];
  rstd = sh[1];
  __syncthreads();
}

__device__ __forceinline__ void gln_mean_rstd(const double* __restrict__ part, int nparts, double* sh, float& mean, float& rstd) {
  double mu, rs;
  gln_mean_rstd_f64(part, nparts, sh, mu, rs);
  mean = (float)mu;
  rstd = (float)rs;
}

__device__ __forceinline__ float prelu(float v, float a) { return v >= 0.0f ? v : a * v; }

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// shape checks shared by the three elementwise entry points
static int check_tiles(int64_t M, int64_t K, int32_t C, int64_t* tiles) {
  if (M < 1 || K < 1 || C < 1) return MA_ERR_INVALID_ARG;
  if (C % 64 != 0 || C > kTnTileElems) return MA_ERR_UNSUPPORTED;
  *tiles = (K + tile_rows(C) - 1) / tile_rows(C);
  if (M > 65535 || *tiles > 0x7fffffff || M * K > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  return MA_OK;
}

}  // namespace ma
