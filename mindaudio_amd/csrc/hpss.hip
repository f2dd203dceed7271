// Harmonic / percussive separation of mindaudio/data/features.py (soft_mask :438-469, hpss :472-529): the 1-D median filter the
// reference takes from scipy.ndimage, and the mask arithmetic.  Contract: include/mindaudio_amd.h.
//
//   1. median_filter_kernel: x as a strided view (rows, n, inner), the filter along n.  A workgroup owns kMedSeg outputs of each of
//      L neighbouring lines (lines that differ in the `inner` index) and stages their kMedSeg + k - 1 inputs in LDS with the periodic
//      half-sample reflection applied, so the filter itself never leaves LDS.  Two shapes of the same tile, chosen by which stride
//      is the small one:
//        along n   (the line is contiguous):  L = 4, a wave per line, a lane per output; LDS [line][position].
//        along inner (the lines are interleaved): L = 256 bytes' worth of lines, a lane per line; LDS [position][line].
//      In both, global reads and writes of a wave run along the unit stride and the 64 lanes of a wave read 64 consecutive LDS words
//      (ds_read_b32: two groups of 32 lanes on 32 banks, no conflict), and the staging stores are consecutive words too.
//      Each thread picks the median of its window by rank counting: candidate j wins when
//        #(w[m] <= w[j], m < j) + #(w[m] < w[j], m > j) == k / 2,
//      which exactly one j satisfies whatever the ties: a selection, no arithmetic on the values.  O(k^2) compares per output.
//      Inputs are finite; what comes out of a window that holds a NaN is not specified.
//   2. soft_mask_kernel: one thread per element, the reference's operations in its order, in the array's type, every one a
//      correctly rounded IEEE operation: the file is compiled with contraction off (x * x + y must stay a product and a sum, as in
//      NumPy), and division and square root are the compiler's IEEE forms (no fast-math flag is given to this library).
//      The "any input negative" flag is a plain store of 1 by every thread that sees one.
//   3. stft_frames_kernel: the windowed, padded frames of a waveform as complex rows (imaginary part 0), the input of the
//      power-of-two FFT (ma_fft_pow2_c32) for the n_fft that the fused stft kernels do not cover - harmonic's n_fft = 2048.
//   4. istft_rows_kernel / istft_ola_rows_kernel: the way back for the same n_fft.  ma_istft_f32 sums a frame's n_fft / 2 terms one
//      after the other in float32, which at n_fft = 2048 costs several times the rounding error of the rest of harmonic; here a
//      frame's Hermitian spectrum is laid out as a complex row for the inverse power-of-two FFT, and the overlap-add (ma_istft_f32's,
//      term for term) reads the real parts.
//
// No atomics and no order-dependent arithmetic: the same bits from run to run, and for a row alone or inside a batch.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

#pragma clang fp contract(off)

namespace ma {

constexpr int kMedThreads = 256;
constexpr int kMedSeg = MA_MEDIAN_SEGMENT;  // outputs of a line per workgroup
constexpr int kMedMaxK = MA_MEDIAN_MAX_K;
constexpr int kMedLinesAlongN = kMedThreads / kMedSeg;
static_assert(kMedSeg == 64, "a wave covers one segment of a line");

// lines per workgroup where the lanes run along `inner`: 256 bytes of neighbouring lines
template <typename T>
constexpr int med_lines_along_inner() {
  return 256 / (int)sizeof(T);
}
template <typename T, bool kAlongN>
constexpr int med_lines() {
  return kAlongN ? kMedLinesAlongN : med_lines_along_inner<T>();
}
// (kMedSeg + kMedMaxK - 1) * 64 * 4 = 48640 bytes at most: under the 64 KiB a kernel gets without an attribute
static size_t med_lds_bytes(int lines, int k, size_t elem) { return (size_t)(kMedSeg + k - 1) * lines * elem; }

// index j (any integer) of a line of n elements under scipy's mode="reflect": d c b a | a b c d | d c b a, periodic in 2n
__device__ __forceinline__ int64_t reflect_index(int64_t j, int64_t n) {
  const int64_t period = 2 * n;
  int64_t r = j % period;
  if (r < 0) r += period;
  return r < n ? r : period - 1 - r;
}

template <typename T, bool kAlongN>
__global__ __launch_bounds__(kMedThreads) void median_filter_kernel(const T* __restrict__ x, int64_t n, int64_t inner, int64_t xs_r,
                                                                    int64_t xs_n, int64_t xs_i, int k, T* __restrict__ out,
                                                                    int64_t os_r, int64_t os_n, int64_t os_i, int tiles_n,
                                                                    int64_t tiles_l) {
  extern __shared__ __attribute__((aligned(16))) unsigned char med_lds[];
  T* w = reinterpret_cast<T*>(med_lds);
  constexpr int L = med_lines<T, kAlongN>();
  const int W = kMedSeg + k - 1;  // staged positions of a line
  // LDS address of (line l, staged position j)
  const int sl = kAlongN ? W : 1, sj = kAlongN ? 1 : L;

  const int64_t bid = blockIdx.x;
  const int tn = (int)(bid % tiles_n);
  const int64_t rest = bid / tiles_n;
  const int64_t tl = rest % tiles_l, row = rest / tiles_l;
  const int64_t p0 = (int64_t)tn * kMedSeg;  // first output position of the tile
  const int64_t c0 = tl * L;                 // first line (inner index) of the tile
  const T* xr = x + row * xs_r;
  T* orow = out + row * os_r;

  // ---- stage: the fast thread index runs along the unit stride ----
  const int total = L * W;
  for (int e = threadIdx.x; e < total; e += kMedThreads) {
    const int l = kAlongN ? e / W : e % L;
    const int j = kAlongN ? e % W : e / L;
    const int64_t c = c0 + l;
    T v = (T)0;
    if (c < inner) v = xr[reflect_index(p0 - k / 2 + j, n) * xs_n + c * xs_i];
    w[l * sl + j * sj] = v;
  }
  __syncthreads();

  // ---- select ----
  const int rank = k / 2;
  constexpr int per_pass = kMedThreads / L;  // positions a pass of the workgroup covers (along inner); along n one pass covers all
  const int l = kAlongN ? (int)threadIdx.x / kMedSeg : (int)threadIdx.x % L;
  const int pfirst = kAlongN ? (int)threadIdx.x % kMedSeg : (int)threadIdx.x / L;
  const int pstep = kAlongN ? kMedSeg : per_pass;
  const int64_t c = c0 + l;
  for (int p = pfirst; p < kMedSeg; p += pstep) {
    if (c >= inner || p0 + p >= n) continue;  // (nothing below synchronises)
    const T* win = w + l * sl + p * sj;
    T res = win[0];
    for (int j = 0; j < k; ++j) {
      const T v = win[j * sj];
      int cnt = 0;
      // (unroll 8: left alone the compiler pairs the loads of the along-n form only; measured)
#pragma unroll 8
      for (int m = 0; m < j; ++m) cnt += win[m * sj] <= v ? 1 : 0;
#pragma unroll 8
      for (int m = j + 1; m < k; ++m) cnt += win[m * sj] < v ? 1 : 0;
      res = cnt == rank ? v : res;
    }
    orow[(p0 + p) * os_n + c * os_i] = res;
  }
}

template <typename T, bool kAlongN>
static int median_launch(const void* x, int64_t rows, int64_t n, int64_t inner, int64_t xs_r, int64_t xs_n, int64_t xs_i, int k,
                         void* out, int64_t os_r, int64_t os_n, int64_t os_i, hipStream_t stream) {
  constexpr int L = med_lines<T, kAlongN>();
  const int64_t tiles_n = (n + kMedSeg - 1) / kMedSeg, tiles_l = (inner + L - 1) / L;
  if (tiles_n > 0x7fffffff || tiles_l > 0x7fffffff || rows > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  // (three factors below 2^31 each: the first product cannot overflow 64 bits, the second is checked by division)
  const int64_t per_row = tiles_n * tiles_l;
  if (per_row > 0x7fffffff || rows > 0x7fffffff / per_row) return MA_ERR_UNSUPPORTED;
  const size_t lds = med_lds_bytes(L, k, sizeof(T));
  MA_LAUNCH((median_filter_kernel<T, kAlongN>), dim3((unsigned)(rows * per_row)), dim3(kMedThreads), lds, stream,
            static_cast<const T*>(x), n, inner, xs_r, xs_n, xs_i, k, static_cast<T*>(out), os_r, os_n, os_i, (int)tiles_n, tiles_l);
  return MA_OK;
}

// ---- soft mask ------------------------------------------------------------------------------------------------------------------------
enum { kPowGeneric = 0, kPowOne = 1, kPowTwo = 2, kPowHalf = 3, kPowInf = 4 };

template <typename T>
__device__ __forceinline__ T tiny_of();
template <>
__device__ __forceinline__ float tiny_of<float>() { return FLT_MIN; }
template <>
__device__ __forceinline__ double tiny_of<double>() { return DBL_MIN; }

__device__ __forceinline__ float pow_t(float v, float p) { return powf(v, p); }
__device__ __forceinline__ double pow_t(double v, double p) { return pow(v, p); }
__device__ __forceinline__ float sqrt_t(float v) { return sqrtf(v); }
__device__ __forceinline__ double sqrt_t(double v) { return sqrt(v); }

template <typename T>
__device__ __forceinline__ T raise_to(T v, int mode, T power) {
  switch (mode) {
    case kPowOne: return v;
    case kPowTwo: return v * v;
    case kPowHalf: return sqrt_t(v);
    default: return pow_t(v, power);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void soft_mask_kernel(const T* __restrict__ a, const T* __restrict__ b, int64_t count, T scale_a,
                                                        T scale_b, int mode, T power, int split_zeros, void* __restrict__ mask,
                                                        const T* __restrict__ spec, const float* __restrict__ phase,
                                                        void* __restrict__ out, int32_t* __restrict__ negative) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const T x = a[i] * scale_a, r = b[i] * scale_b;
  if (negative && (x < (T)0 || r < (T)0)) *negative = 1;
  T m;
  if (mode == kPowInf) {
    m = x > r ? (T)1 : (T)0;
    if (mask) static_cast<uint8_t*>(mask)[i] = x > r ? 1 : 0;
  } else {
    T z = x > r ? x : r;  // np.maximum of finite values
    const bool bad = z < tiny_of<T>();
    z = bad ? (T)1 : z;
    m = raise_to(x / z, mode, power);
    const T rm = raise_to(r / z, mode, power);
    const T sum = m + rm;
    m = bad ? (split_zeros ? (T)0.5 : (T)0) : m / sum;
    if (mask) static_cast<T*>(mask)[i] = m;
  }
  if (out) {
    const T s = spec[i] * m;
    if (phase) {  // (float only: checked by the entry)
      float* o = static_cast<float*>(out);
      o[2 * i] = (float)s * phase[2 * i];
      o[2 * i + 1] = (float)s * phase[2 * i + 1];
    } else {
      static_cast<T*>(out)[i] = s;
    }
  }
}

template <typename T>
static int soft_mask_launch(const void* a, const void* b, int64_t count, double scale_a, double scale_b, int mode, double power,
                            int split_zeros, void* mask, const void* spec, const void* phase, void* out, int32_t* negative,
                            hipStream_t stream) {
  const int64_t blocks = (count + 255) / 256;
  if (blocks > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(soft_mask_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const T*>(a), static_cast<const T*>(b),
            count, (T)scale_a, (T)scale_b, mode, (T)power, split_zeros, mask, static_cast<const T*>(spec),
            static_cast<const float*>(phase), out, negative);
  return MA_OK;
}

// ---- frames for the large-n_fft stft --------------------------------------------------------------------------------------------------
// sample index of padded position i under np.pad's modes (one reflection: the pad is n_fft / 2 <= n / 2); -1: a zero
__device__ __forceinline__ int64_t padded_index(int64_t i, int64_t n, int mode) {
  if (i >= 0 && i < n) return i;
  if (mode == MA_PAD_CONSTANT) return -1;
  int64_t r;
  if (mode == MA_PAD_REFLECT) r = i < 0 ? -i : 2 * (n - 1) - i;
  else if (mode == MA_PAD_SYMMETRIC) r = i < 0 ? -i - 1 : 2 * n - 1 - i;
  else r = i;  // edge
  return r < 0 ? 0 : (r >= n ? n - 1 : r);
}

__global__ __launch_bounds__(256) void stft_frames_kernel(const float* __restrict__ x, int64_t n, int64_t ldx, int n_fft, int hop,
                                                          const float* __restrict__ window, int pad, int pad_mode, int64_t n_frames,
                                                          float2* __restrict__ frames) {
  const int64_t f = blockIdx.x, b = blockIdx.y;
  const float* xr = x + b * ldx;
  float2* fr = frames + (b * n_frames + f) * n_fft;
  for (int i = threadIdx.x; i < n_fft; i += 256) {
    const int64_t s = padded_index(f * hop - pad + i, n, pad_mode);
    const float v = s < 0 ? 0.0f : xr[s];
    fr[i] = make_float2(v * window[i], 0.0f);
  }
}

// spec (batch, n_freq, frames_total) bin-major -> rows (batch, n_frames, N): S_k for k <= N / 2 and conj(S_{N - k}) above it, the
// imaginary parts of the DC and Nyquist bins dropped (as the C2R transform behind numpy.fft.irfft does)
__global__ __launch_bounds__(256) void istft_rows_kernel(const float2* __restrict__ spec, int64_t frames_total, int64_t n_frames, int N,
                                                         float2* __restrict__ rows) {
  const int64_t t = blockIdx.x, b = blockIdx.y;
  const int half = N / 2;
  const float2* sb = spec + b * (int64_t)(half + 1) * frames_total + t;
  float2* r = rows + (b * n_frames + t) * N;
  for (int k = threadIdx.x; k <= half; k += 256) {
    const float2 v = sb[(int64_t)k * frames_total];
    if (k == 0 || k == half) {
      r[k] = make_float2(v.x, 0.0f);
    } else {
      r[k] = v;
      r[N - k] = make_float2(v.x, -v.y);
    }
  }
}

// ma_istft_f32's overlap-add on the real parts of the (unnormalised) inverse transforms
__global__ __launch_bounds__(256) void istft_ola_rows_kernel(const float2* __restrict__ rows, const float* __restrict__ win,
                                                             int64_t n_frames, int N, int hop, int start, int64_t out_len,
                                                             float* __restrict__ out) {
  const int64_t exp_len = (int64_t)N + (int64_t)hop * (n_frames - 1);
  const float2* fb = rows + (int64_t)blockIdx.y * n_frames * N;
  float* ob = out + (int64_t)blockIdx.y * out_len;
  const float inv = 1.0f / (float)N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < out_len; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i + start;
    float y = 0.0f, wss = 0.0f;
    if (n < exp_len) {
      int64_t t_hi = n / hop;
      if (t_hi > n_frames - 1) t_hi = n_frames - 1;
      for (int64_t t = t_hi; t >= 0; --t) {
        const int64_t j = n - t * hop;
        if (j >= N) break;
        const float w = win[j];
        y += w * (fb[t * N + j].x * inv);
        wss += w * w;
      }
    }
    ob[i] = wss > 1e-9f ? y / wss : y;
  }
}

}  // namespace ma

using namespace ma;

extern "C" int ma_istft_rows_c32(const float* spec, int64_t batch, int32_t n_fft, int64_t frames_total, int64_t n_frames, float* rows,
                                 ma_stream_t stream) {
  if (!spec || !rows || batch < 1 || n_frames < 1 || frames_total < n_frames) return MA_ERR_INVALID_ARG;
  if (n_fft < 2 || (n_fft & 1) || batch > 65535 || n_frames > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(istft_rows_kernel, dim3((unsigned)n_frames, (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
            reinterpret_cast<const float2*>(spec), frames_total, n_frames, (int)n_fft, reinterpret_cast<float2*>(rows));
  return MA_OK;
}

extern "C" int ma_istft_ola_c32(const float* rows, int64_t batch, int32_t n_fft, int64_t n_frames, int32_t hop, const float* window,
                                int32_t start, float* out, int64_t out_len, ma_stream_t stream) {
  if (!rows || !window || !out || batch < 1 || n_frames < 1 || out_len < 1 || start < 0) return MA_ERR_INVALID_ARG;
  if (hop < 1) return MA_ERR_HOP;
  if (n_fft < 2 || (n_fft & 1) || batch > 65535 || n_frames > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  int64_t blocks = (out_len + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  MA_LAUNCH(istft_ola_rows_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
            reinterpret_cast<const float2*>(rows), window, n_frames, (int)n_fft, (int)hop, (int)start, out_len, out);
  return MA_OK;
}

extern "C" int ma_stft_frames_c32(const float* x, int64_t batch, int64_t n, int64_t ldx, int32_t n_fft, int32_t hop,
                                  const float* window, int32_t center, int32_t pad_mode, float* frames, int64_t n_frames,
                                  ma_stream_t stream) {
  if (!x || !window || !frames || batch < 1 || n < 1 || ldx < n || n_fft < 2) return MA_ERR_INVALID_ARG;
  if (hop < 1) return MA_ERR_HOP;
  if (n_fft > n) return MA_ERR_NFFT_TOO_LARGE;
  if (pad_mode < MA_PAD_CONSTANT || pad_mode > MA_PAD_SYMMETRIC) return MA_ERR_INVALID_ARG;
  if (n_frames != ma_num_frames(n, n_fft, hop, center)) return MA_ERR_INVALID_ARG;
  if (batch > 65535 || n_frames > 0x7fffffff) return MA_ERR_UNSUPPORTED;
  MA_LAUNCH(stft_frames_kernel, dim3((unsigned)n_frames, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x, n, ldx, (int)n_fft,
            (int)hop, window, center ? n_fft / 2 : 0, (int)pad_mode, n_frames, reinterpret_cast<float2*>(frames));
  return MA_OK;
}

extern "C" int ma_median_filter(const void* x, int32_t dtype, int64_t rows, int64_t n, int64_t inner, int64_t x_stride_rows,
                                int64_t x_stride_n, int64_t x_stride_inner, int32_t k, void* out, int64_t out_stride_rows,
                                int64_t out_stride_n, int64_t out_stride_inner, ma_stream_t stream) {
  if (!x || !out || x == out || rows < 1 || n < 1 || inner < 1) return MA_ERR_INVALID_ARG;
  if (dtype != MA_DTYPE_F32 && dtype != MA_DTYPE_F64) return MA_ERR_INVALID_ARG;
  if (k < 1 || k > kMedMaxK || (int64_t)k > 4 * n) return MA_ERR_INVALID_ARG;
  if (x_stride_rows < 0 || x_stride_n < 0 || x_stride_inner < 0 || out_stride_rows < 0 || out_stride_n < 0 || out_stride_inner < 0)
    return MA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  // lanes along n where the line is the denser of the two axes (or the only one)
  const bool along_n = inner == 1 || x_stride_n <= x_stride_inner;
#define MA_MEDIAN_CASE(T, ALONG)                                                                                                      \
  return median_launch<T, ALONG>(x, rows, n, inner, x_stride_rows, x_stride_n, x_stride_inner, (int)k, out, out_stride_rows,         \
                                 out_stride_n, out_stride_inner, s)
  if (dtype == MA_DTYPE_F32) {
    if (along_n) MA_MEDIAN_CASE(float, true);
    MA_MEDIAN_CASE(float, false);
  }
  if (along_n) MA_MEDIAN_CASE(double, true);
  MA_MEDIAN_CASE(double, false);
#undef MA_MEDIAN_CASE
}

extern "C" int ma_soft_mask(const void* a, const void* b, int32_t dtype, int64_t count, double scale_a, double scale_b, double power,
                            int32_t split_zeros, void* mask, const void* spec, const void* phase, void* out, int32_t* negative,
                            ma_stream_t stream) {
  if (!a || !b || count < 1 || (!mask && !out) || (out && !spec) || (phase && !out)) return MA_ERR_INVALID_ARG;
  if (dtype != MA_DTYPE_F32 && dtype != MA_DTYPE_F64) return MA_ERR_INVALID_ARG;
  if (phase && dtype != MA_DTYPE_F32) return MA_ERR_INVALID_ARG;
  if (!(power > 0.0)) return MA_ERR_INVALID_ARG;  // (a NaN fails the comparison too)
  const int mode = power == 1.0 ? kPowOne : power == 2.0 ? kPowTwo : power == 0.5 ? kPowHalf : isinf(power) ? kPowInf : kPowGeneric;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MA_DTYPE_F32)
    return soft_mask_launch<float>(a, b, count, scale_a, scale_b, mode, power, split_zeros ? 1 : 0, mask, spec, phase, out, negative,
                                   s);
  return soft_mask_launch<double>(a, b, count, scale_a, scale_b, mode, power, split_zeros ? 1 : 0, mask, spec, phase, out, negative, s);
}
