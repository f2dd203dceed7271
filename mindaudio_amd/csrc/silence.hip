// The silence front end and the channel / axis reductions of mindaudio/data/processing.py (trim, split, normalize,
// stereo_to_mono).  Contract: include/mindaudio_amd.h.
//
// The reference frames the zero-padded signal into a float64 array frame_length / hop_length times its size (a Python loop of
// frame_length iterations), takes mean(x^2) per frame, turns that into decibels against a reference and reads the non-silent
// edges off a diff.  Here:
//   1. frame_power_kernel: one workgroup per (row, tile of kFpTile frames).  Where hop_length divides frame_length (R = their
//      ratio <= kFpMaxR) the tile's R + kFpTile - 1 hop blocks are summed once, a wave per block, into LDS and a frame is the sum
//      of its R block sums in index order: a sample is read once (plus the R - 1 blocks two neighbouring tiles share).  Otherwise
//      a wave sums a frame directly.  Samples are not staged: a wave reads a run of consecutive samples, once.
//   2. row_max_kernel: one workgroup per row over its frames (a maximum has no order to fix).
//   3. silence_edges_kernel: one workgroup per row.  flag(f) in float64; a boundary sits at i in [0, F] where flag(i - 1) !=
//      flag(i) (both ends count as silent), boundaries are compacted by a ballot / popcount prefix scan, 256 positions at a time.
//      The first boundary is trim's start, the last one its end; consecutive pairs are split's intervals.
//   4. axis_stats_kernel: x as (outer, n, inner); a workgroup owns up to 64 neighbouring `inner` columns of one outer index and
//      cuts n into 256 / columns slices, one thread per (slice, column) - inner == 1 is 256 slices of a contiguous row, a wide
//      inner is four slices of 64 coalesced columns.  Slices are joined by a tree in LDS.
//      axis_apply_kernel then forms (x - mean) / scale per element in float64 and rounds once more to the output's type.
//   5. channel_mean_kernel: one thread per sample, the channels added in NumPy's order in the input's type.
//
// Every sum has an order that depends on the shape alone (a lane strides by 64, waves join by the xor butterfly, slices by a
// halving tree): no atomics, the same bits from run to run, and - a tile starts at a multiple of kFpTile frames whatever the
// batch, and the zeros behind a row's length add exactly - for a row alone or inside a ragged batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kFpThreads = 256;
constexpr int kFpWaves = kFpThreads / 64;
constexpr int kFpTile = MA_FRAME_POWER_TILE;  // frames per workgroup
constexpr int kFpMaxR = MA_FRAME_POWER_MAX_RATIO;
static_assert(kFpTile <= kFpThreads, "one thread per frame of a tile");

// frames of a row of n samples: the reference's (n + 2 pad - frame_length) // hop + 1 with pad = frame_length // 2
__host__ __device__ inline int64_t frames_of(int64_t n, int frame_length, int hop) {
  return n < 1 ? 0 : (n - (frame_length & 1)) / hop + 1;
}

// sum of x[s]^2 over the padded positions [p0, p0 + len) (sample s = position - pad, zero outside [0, n)); every lane returns it
template <typename S>
__device__ __forceinline__ double span_power(const S* __restrict__ row, int64_t n, int64_t p0, int len, int pad, int lane) {
  double acc = 0.0;
  for (int i = lane; i < len; i += 64) {
    const int64_t s = p0 - pad + i;
    if (s >= 0 && s < n) {
      const double v = (double)row[s];
      acc = fma(v, v, acc);
    }
  }
  return wave_sum(acc);
}

template <typename S>
__global__ __launch_bounds__(kFpThreads) void frame_power_kernel(const S* __restrict__ x, int64_t ldx, int64_t T,
                                                                 const int32_t* __restrict__ lengths, int frame_length, int hop,
                                                                 int ratio, int tiles, double* __restrict__ power, int64_t ldp) {
  __shared__ double block_sum[kFpTile + kFpMaxR - 1];
  const int64_t row = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - row * tiles);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t n = lengths ? (int64_t)lengths[row] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const int64_t F = frames_of(n, frame_length, hop);
  const int64_t f0 = (int64_t)tile * kFpTile;
  const int pad = frame_length / 2;
  const S* xr = x + row * ldx;
  double* pr = power + row * ldp;
  const double inv = (double)frame_length;
  if (ratio > 0) {
    const int nb = kFpTile + ratio - 1;
    for (int j = wave; j < nb; j += kFpWaves) {
      const double s = f0 + j < F + ratio - 1 ? span_power(xr, n, (f0 + j) * hop, hop, pad, lane) : 0.0;
      if (lane == 0) block_sum[j] = s;
    }
    __syncthreads();
    const int f = threadIdx.x;
    if (f < kFpTile && f0 + f < ldp) {
      double acc = 0.0;
      if (f0 + f < F) {
        for (int j = 0; j < ratio; ++j) acc += block_sum[f + j];
        const double r = sqrt(acc / inv);
        acc = r * r;
      }
      pr[f0 + f] = acc;
    }
  } else {
    for (int f = wave; f < kFpTile; f += kFpWaves) {
      if (f0 + f >= ldp) break;
      double acc = 0.0;
      if (f0 + f < F) {
        const double r = sqrt(span_power(xr, n, (f0 + f) * hop, frame_length, pad, lane) / inv);
        acc = r * r;
      }
      if (lane == 0) pr[f0 + f] = acc;
    }
  }
}

__global__ __launch_bounds__(kFpThreads) void row_max_kernel(const double* __restrict__ power, int64_t ldp, int64_t T,
                                                             const int32_t* __restrict__ lengths, int frame_length, int hop,
                                                             double* __restrict__ row_max) {
  __shared__ double part[kFpThreads];
  const int64_t row = blockIdx.x;
  int64_t n = lengths ? (int64_t)lengths[row] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const int64_t F = frames_of(n, frame_length, hop);
  double m = 0.0;  // a power is never negative
  for (int64_t f = threadIdx.x; f < F; f += kFpThreads) {
    const double p = power[row * ldp + f];
    m = (p > m || p != p) ? p : m;
  }
  part[threadIdx.x] = m;
  __syncthreads();
  for (int h = kFpThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      const double a = part[threadIdx.x], b = part[threadIdx.x + h];
      part[threadIdx.x] = (b > a || b != b) ? b : a;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) row_max[row] = part[0];
}

__global__ __launch_bounds__(kFpThreads) void silence_edges_kernel(const double* __restrict__ power, int64_t ldp, int64_t T,
                                                                   const int32_t* __restrict__ lengths, int frame_length, int hop,
                                                                   const double* __restrict__ ref_rows, double ref_scalar,
                                                                   double top_db, int64_t clip, uint8_t* __restrict__ nonsilent,
                                                                   int32_t* __restrict__ trim_index, int32_t* __restrict__ counts,
                                                                   int32_t* __restrict__ edges) {
  __shared__ int wave_count[kFpWaves];
  __shared__ int64_t first_b, last_b;
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t n = lengths ? (int64_t)lengths[row] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const int64_t F = frames_of(n, frame_length, hop);
  const int64_t lim = clip >= 0 ? clip : n;
  const double* pr = power + row * ldp;
  const double ref = ref_rows ? ref_rows[row] : ref_scalar;
  const double ref_db = 10.0 * log10(fmax(1e-10, ref));
  auto flag = [&](int64_t f) -> bool {
    if (f < 0 || f >= F) return false;
    return 10.0 * log10(fmax(pr[f], 1e-10)) - ref_db > -top_db;
  };
  if (threadIdx.x == 0) first_b = last_b = -1;
  for (int64_t f = threadIdx.x; f < ldp; f += kFpThreads) nonsilent[row * ldp + f] = flag(f) ? 1 : 0;
  int32_t* er = edges + row * (ldp + 1);
  int64_t base = 0;  // boundaries before this pass (the same value in every thread)
  for (int64_t i0 = 0; i0 <= F; i0 += kFpThreads) {
    const int64_t i = i0 + threadIdx.x;
    const bool b = i <= F && flag(i - 1) != flag(i);
    const unsigned long long mask = __ballot(b);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kFpWaves; ++w) {
      before += w < wave ? wave_count[w] : 0;
      total += wave_count[w];
    }
    const int rank = before + __popcll(mask & ((1ull << lane) - 1ull));
    if (b) {
      const int64_t pos = i * hop;
      er[base + rank] = (int32_t)(pos < lim ? pos : lim);
      if (base + rank == 0) first_b = i;
      if (rank == total - 1) last_b = i;  // (a later pass overwrites it)
    }
    base += total;
    __syncthreads();
  }
  for (int64_t e = base + threadIdx.x; e < ldp + 1; e += kFpThreads) er[e] = -1;
  if (threadIdx.x == 0) {
    counts[row] = (int32_t)(base / 2);
    trim_index[2 * row] = base ? (int32_t)(first_b * hop) : -1;
    trim_index[2 * row + 1] = base ? (int32_t)(last_b * hop) : -1;  // not clipped: the reference's trim does not clip it
  }
}

// ---- axis statistics ----------------------------------------------------------------------------------------------------------------
constexpr int kAxThreads = 256;
constexpr int kAxMaxCols = 64;

template <typename S>
__device__ __forceinline__ double magnitude(S v) {
  if constexpr (std::is_floating_point<S>::value) {
    return fabs((double)v);
  } else {
    return (double)(v < 0 ? -v : v);
  }
}

// NaN wins, as in np.max / np.min
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }

// One pass of a thread over its slice.  kind: 0 max, 1 min, 2 sum of f(v)
template <typename S, class F>
__device__ __forceinline__ double axis_pass(const S* __restrict__ col, int64_t n, int64_t inner, int slice, int slices, int kind,
                                            F&& f) {
  double acc = kind == 0 ? -INFINITY : kind == 1 ? INFINITY : 0.0;
  for (int64_t k = slice; k < n; k += slices) {
    const double m = magnitude(col[k * inner]);
    acc = kind == 0 ? nan_max(acc, m) : kind == 1 ? nan_min(acc, m) : acc + f(m);
  }
  return acc;
}

// joins the slices' partials; every thread returns column c's result
__device__ __forceinline__ double axis_join(double* part, double v, int slice, int slices, int c, int cw, int kind) {
  part[slice * cw + c] = v;
  __syncthreads();
  for (int h = slices / 2; h > 0; h >>= 1) {
    if (slice < h) {
      const double a = part[slice * cw + c], b = part[(slice + h) * cw + c];
      part[slice * cw + c] = kind == 0 ? nan_max(a, b) : kind == 1 ? nan_min(a, b) : a + b;
    }
    __syncthreads();
  }
  const double r = part[c];
  __syncthreads();
  return r;
}

template <typename S>
__global__ __launch_bounds__(kAxThreads) void axis_stats_kernel(const S* __restrict__ x, int64_t n, int64_t inner, int cw,
                                                                int col_tiles, int stat, double* __restrict__ out) {
  __shared__ double part[kAxThreads];
  const int64_t o = blockIdx.x / col_tiles;
  const int64_t c0 = (int64_t)(blockIdx.x - o * col_tiles) * cw;
  const int slices = kAxThreads / cw;
  const int c = threadIdx.x % cw, slice = threadIdx.x / cw;
  const bool live = c0 + c < inner;
  const S* col = x + o * n * inner + (live ? c0 + c : 0);
  const int64_t rows = live ? n : 0;
  double r;
  if (stat == MA_AXIS_MAX || stat == MA_AXIS_MIN) {
    const int kind = stat == MA_AXIS_MAX ? 0 : 1;
    r = axis_join(part, axis_pass(col, rows, inner, slice, slices, kind, [](double m) { return m; }), slice, slices, c, cw, kind);
  } else if (stat == MA_AXIS_L0) {
    r = axis_join(part, axis_pass(col, rows, inner, slice, slices, 2, [](double m) { return m > 0.0 ? 1.0 : 0.0; }), slice, slices,
                  c, cw, 2);
  } else if (stat == MA_AXIS_SUMSQ) {
    r = axis_join(part, axis_pass(col, rows, inner, slice, slices, 2, [](double m) { return m * m; }), slice, slices, c, cw, 2);
  } else {
    r = axis_join(part, axis_pass(col, rows, inner, slice, slices, 2, [](double m) { return m; }), slice, slices, c, cw, 2);
    if (stat != MA_AXIS_SUM) r = r / (double)n;
    if (stat == MA_AXIS_STD) {  // the two-pass form of np.std
      const double mean = r;
      r = axis_join(part, axis_pass(col, rows, inner, slice, slices, 2, [mean](double m) { return (m - mean) * (m - mean); }),
                    slice, slices, c, cw, 2);
      r = sqrt(r / (double)n);
    }
  }
  if (slice == 0 && live) out[o * inner + c0 + c] = r;
}

// out = (x - sub) / div in float64, each of sub and div (outer, inner) float64 or absent; the result is converted to O (an
// integer O truncates toward zero, as the reference's assignment into np.empty_like does)
template <typename S, typename O>
__global__ __launch_bounds__(256) void axis_apply_kernel(const S* __restrict__ x, int64_t total, int64_t n, int64_t inner,
                                                         const double* __restrict__ sub, const double* __restrict__ div,
                                                         O* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t s = (i / (n * inner)) * inner + i % inner;  // the statistic's slot
  double v = (double)x[i];
  if (sub) v -= sub[s];
  if (div) v /= div[s];
  out[i] = (O)v;
}

// ---- channel mean ---------------------------------------------------------------------------------------------------------------------
// NumPy's add.reduce over a contiguous axis of C elements: in index order below 8, and at 8 the pairs of its unrolled block.
template <typename S>
__global__ __launch_bounds__(256) void channel_mean_kernel(const S* __restrict__ x, int64_t n, int C, S* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const S* p = x + i * C;
  S acc;
  if (C == 8) {
    acc = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
  } else {
    acc = p[0];
    for (int c = 1; c < C; ++c) acc += p[c];
  }
  out[i] = acc / (S)C;
}

static bool silence_shape_ok(int64_t B, int64_t T, int frame_length, int hop) {
  return B >= 1 && T >= 1 && frame_length >= 1 && hop >= 1;
}
// positions and edges are int32 on the way out
static bool silence_shape_built(int64_t B, int64_t T, int frame_length, int hop) {
  return T + (int64_t)hop + frame_length < 0x7fffff00LL && B <= 0x7fffffff;
}

template <typename S>
static int frame_power_launch(const S* x, int64_t ldx, int64_t B, int64_t T, const int32_t* lengths, int frame_length, int hop,
                              double* power, int64_t ldp, double* row_max, hipStream_t stream) {
  const int ratio = frame_length % hop == 0 && frame_length / hop <= kFpMaxR ? frame_length / hop : 0;
  const int64_t tiles = (ldp + kFpTile - 1) / kFpTile;
  if (B * tiles > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH((frame_power_kernel<S>), dim3((unsigned)(B * tiles)), dim3(kFpThreads), 0, stream, x, ldx, T, lengths, frame_length,
            hop, ratio, (int)tiles, power, ldp);
  MA_LAUNCH(row_max_kernel, dim3((unsigned)B), dim3(kFpThreads), 0, stream, power, ldp, T, lengths, frame_length, hop, row_max);
  return MA_OK;
}

template <typename S>
static int axis_stats_launch(const void* x, int64_t outer, int64_t n, int64_t inner, int stat, double* out, hipStream_t stream) {
  int cw = 1;
  while (cw < kAxMaxCols && cw < inner) cw *= 2;
  const int64_t col_tiles = (inner + cw - 1) / cw;
  if (outer * col_tiles > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH((axis_stats_kernel<S>), dim3((unsigned)(outer * col_tiles)), dim3(kAxThreads), 0, stream, static_cast<const S*>(x), n,
            inner, cw, (int)col_tiles, stat, out);
  return MA_OK;
}

template <typename S>
static int axis_apply_launch(const void* x, int64_t outer, int64_t n, int64_t inner, const double* sub, const double* div, void* out,
                             int out_dtype, hipStream_t stream) {
  const int64_t total = outer * n * inner, blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  const S* xs = static_cast<const S*>(x);
  if (out_dtype == MA_DTYPE_F64)
    MA_LAUNCH((axis_apply_kernel<S, double>), dim3((unsigned)blocks), dim3(256), 0, stream, xs, total, n, inner, sub, div,
              static_cast<double*>(out));
  else
    MA_LAUNCH((axis_apply_kernel<S, S>), dim3((unsigned)blocks), dim3(256), 0, stream, xs, total, n, inner, sub, div,
              static_cast<S*>(out));
  return MA_OK;
}

}  // namespace ma

using namespace ma;

extern "C" int64_t ma_frame_power_frames(int64_t n, int32_t frame_length, int32_t hop_length) {
  if (n < 1 || frame_length < 1 || hop_length < 1) return MA_ERR_INVALID_ARG;
  return frames_of(n, frame_length, hop_length);
}

extern "C" int ma_frame_power(const void* x, int32_t sample_bytes, int64_t B, int64_t T, int64_t ldx, const int32_t* lengths,
                              int32_t frame_length, int32_t hop_length, double* power, int64_t ldp, double* row_max,
                              ma_stream_t stream) {
  if (!x || !power || !row_max || (sample_bytes != 4 && sample_bytes != 8)) return MA_ERR_INVALID_ARG;
  if (!silence_shape_ok(B, T, frame_length, hop_length) || ldx < T) return MA_ERR_INVALID_ARG;
  if (!silence_shape_built(B, T, frame_length, hop_length)) return MA_ERR_UNSUPPORTED;
  if (ldp < frames_of(T, frame_length, hop_length)) return MA_ERR_INVALID_ARG;
  if (sample_bytes == 4)
    return frame_power_launch(static_cast<const float*>(x), ldx, B, T, lengths, frame_length, hop_length, power, ldp, row_max,
                              (hipStream_t)stream);
  return frame_power_launch(static_cast<const double*>(x), ldx, B, T, lengths, frame_length, hop_length, power, ldp, row_max,
                            (hipStream_t)stream);
}

extern "C" int ma_silence_edges(const double* power, int64_t ldp, int64_t B, int64_t T, const int32_t* lengths,
                                int32_t frame_length, int32_t hop_length, const double* ref_rows, double ref_scalar, double top_db,
                                int64_t clip, uint8_t* nonsilent, int32_t* trim_index, int32_t* counts, int32_t* edges,
                                ma_stream_t stream) {
  if (!power || !nonsilent || !trim_index || !counts || !edges) return MA_ERR_INVALID_ARG;
  if (!silence_shape_ok(B, T, frame_length, hop_length)) return MA_ERR_INVALID_ARG;
  if (!silence_shape_built(B, T, frame_length, hop_length)) return MA_ERR_UNSUPPORTED;
  if (ldp < frames_of(T, frame_length, hop_length) || clip > 0x7fffffff) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(silence_edges_kernel, dim3((unsigned)B), dim3(kFpThreads), 0, (hipStream_t)stream, power, ldp, T, lengths, frame_length,
            hop_length, ref_rows, ref_scalar, top_db, clip, nonsilent, trim_index, counts, edges);
  return MA_OK;
}

extern "C" int ma_axis_stats(const void* x, int32_t dtype, int64_t outer, int64_t n, int64_t inner, int32_t stat, double* out,
                             ma_stream_t stream) {
  if (!x || !out || outer < 1 || n < 1 || inner < 1) return MA_ERR_INVALID_ARG;
  if (stat < MA_AXIS_MAX || stat > MA_AXIS_STD) return MA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case MA_DTYPE_F32: return axis_stats_launch<float>(x, outer, n, inner, stat, out, s);
    case MA_DTYPE_F64: return axis_stats_launch<double>(x, outer, n, inner, stat, out, s);
    case MA_DTYPE_I32: return axis_stats_launch<int32_t>(x, outer, n, inner, stat, out, s);
    case MA_DTYPE_I64: return axis_stats_launch<int64_t>(x, outer, n, inner, stat, out, s);
    default: return MA_ERR_INVALID_ARG;
  }
}

extern "C" int ma_axis_apply(const void* x, int32_t dtype, int64_t outer, int64_t n, int64_t inner, const double* sub,
                             const double* div, void* out, int32_t out_dtype, ma_stream_t stream) {
  if (!x || !out || outer < 1 || n < 1 || inner < 1 || (!sub && !div)) return MA_ERR_INVALID_ARG;
  if (dtype < MA_DTYPE_F32 || dtype > MA_DTYPE_I64 || (out_dtype != dtype && out_dtype != MA_DTYPE_F64)) return MA_ERR_INVALID_ARG;
  if (x == out) return MA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case MA_DTYPE_F32: return axis_apply_launch<float>(x, outer, n, inner, sub, div, out, out_dtype, s);
    case MA_DTYPE_F64: return axis_apply_launch<double>(x, outer, n, inner, sub, div, out, out_dtype, s);
    case MA_DTYPE_I32: return axis_apply_launch<int32_t>(x, outer, n, inner, sub, div, out, out_dtype, s);
    default: return axis_apply_launch<int64_t>(x, outer, n, inner, sub, div, out, out_dtype, s);
  }
}

extern "C" int ma_channel_mean(const void* x, int32_t sample_bytes, int64_t n, int32_t channels, void* out, ma_stream_t stream) {
  if (!x || !out || n < 1 || channels < 1 || (sample_bytes != 4 && sample_bytes != 8)) return MA_ERR_INVALID_ARG;
  if (channels > MA_CHANNEL_MEAN_MAX) return MA_ERR_UNSUPPORTED;
  const int64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  if (sample_bytes == 4)
    MA_LAUNCH(channel_mean_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, static_cast<const float*>(x),
              n, (int)channels, static_cast<float*>(out));
  else
    MA_LAUNCH(channel_mean_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
              static_cast<const double*>(x), n, (int)channels, static_cast<double*>(out));
  return MA_OK;
}
