// Fixed-order sums of partial results (gfx950): out (+)= alpha * sum_k part[k].  The partials are the split-K products and partial
// column sums of the weight-gradient GEMMs (gemm_tn_bf16.hip, gemm_tn8_bf16.hip, the split-K entry of gemm_bf16.hip) and the
// per-workgroup partials of every parameter reduction of the training paths (LayerNorm, depthwise convolution, attention biases,
// PReLU slopes, basis, encoder).  No atomics: the same bits from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "launch.h"
#include "reduce_splits.h"

namespace ma {

// out[m][n] (+)= alpha * sum_s part[s][m][n]
__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ part, int splits, int64_t mn,
                                                        float* __restrict__ out, int64_t ldo, int N, float alpha,
                                                        int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < mn; i += (int64_t)gridDim.x * 256) {
    float s = 0.0f;
    for (int k = 0; k < splits; ++k) s += part[(int64_t)k * mn + i];
    const int64_t m = i / N;
    float* o = out + m * ldo + (i - m * N);
    *o = accumulate ? *o + alpha * s : alpha * s;
  }
}

// The split sums of a list of products in one launch (ma_reduce_splits_batch_f32): splits are added in the order k = 0 .. splits - 1.
//   short items (accumulate bit 1 clear; weight-gradient splits, a handful of partials of many elements): workgroup b owns 1024
//     consecutive elements of item block_item[b], one thread per 4 elements;
//   tall items (accumulate bit 1 set; per-workgroup partials of a parameter reduction: hundreds of partials of a few hundred
//     elements): workgroup b owns 16 consecutive elements, thread (tx = 4 elements, ty = one of 64 groups of partials) adds the
//     partials ty, ty + 64, ... in order and the 64 group sums are added in order through LDS - a fixed order either way.
__global__ __launch_bounds__(256) void tn_reduce_batch_kernel(const ma_reduce_item_t* __restrict__ items,
                                                              const int32_t* __restrict__ block_item) {
  __shared__ float4 red[64][4];
  const ma_reduce_item_t it = items[block_item[blockIdx.x]];
  const int64_t ps = it.pstride ? (int64_t)it.pstride : it.mn;
  const bool acc = it.accumulate & 1, tall = it.accumulate & 2;
  const bool vec = !(it.N & 3) && !(it.ldo & 3) && !(it.mn & 3) && !(ps & 3) &&
                   !((reinterpret_cast<uintptr_t>(it.out) | reinterpret_cast<uintptr_t>(it.part)) & 15);  // a piece never straddles a row
  auto store4 = [&](int64_t i0, float4 sum) {
    const float v[4] = {sum.x, sum.y, sum.z, sum.w};
    if (vec) {
      const int64_t m = i0 / it.N;
      float4* o = reinterpret_cast<float4*>(it.out + m * it.ldo + (i0 - m * it.N));
      float4 r = make_float4(it.alpha * v[0], it.alpha * v[1], it.alpha * v[2], it.alpha * v[3]);
      if (acc) {
        const float4 old = *o;
        r.x += old.x; r.y += old.y; r.z += old.z; r.w += old.w;
      }
      *o = r;
      return;
    }
    for (int e = 0; e < 4 && i0 + e < it.mn; ++e) {
      const int64_t i = i0 + e, m = i / it.N;
      float* o = it.out + m * it.ldo + (i - m * it.N);
      *o = acc ? *o + it.alpha * v[e] : it.alpha * v[e];
    }
  };
  auto load4 = [&](int64_t k, int64_t i0) -> float4 {
    const float* src = it.part + k * ps + i0;
    if (vec) return *reinterpret_cast<const float4*>(src);
    return make_float4(src[0], i0 + 1 < it.mn ? src[1] : 0.f, i0 + 2 < it.mn ? src[2] : 0.f, i0 + 3 < it.mn ? src[3] : 0.f);
  };
  if (tall) {
    const int tx = threadIdx.x & 3, ty = threadIdx.x >> 2;
    const int64_t i0 = ((int64_t)((int)blockIdx.x - it.first_block) * 4 + tx) * 4;
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i0 < it.mn) {
      // twelve partials of a thread group in flight (the depthwise convolution's 640 partials were ten dependent round trips at four)
      int k = ty;
      for (; k + 11 * 64 < it.splits; k += 12 * 64) {
        float4 v[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) v[u] = load4(k + 64 * u, i0);
#pragma unroll
        for (int u = 0; u < 12; ++u) { sum.x += v[u].x; sum.y += v[u].y; sum.z += v[u].z; sum.w += v[u].w; }
      }
#pragma unroll 4
      for (; k < it.splits; k += 64) {
        const float4 v = load4(k, i0);
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
      }
    }
    red[ty][tx] = sum;
    __syncthreads();
    if (ty == 0 && i0 < it.mn) {
      sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
      for (int k = 0; k < 64; ++k) {
        const float4 v = red[k][tx];
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
      }
      store4(i0, sum);
    }
    return;
  }
  const int64_t i0 = ((int64_t)((int)blockIdx.x - it.first_block) * 256 + threadIdx.x) * 4;
  if (i0 >= it.mn) return;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  int k = 0;
  for (; k + 8 <= it.splits; k += 8) {  // eight partials in flight (the partials are cold: written by GEMMs many launches ago)
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = load4(k + u, i0);
#pragma unroll
    for (int u = 0; u < 8; ++u) { sum.x += v[u].x; sum.y += v[u].y; sum.z += v[u].z; sum.w += v[u].w; }
  }
  for (; k < it.splits; ++k) {
    const float4 v = load4(k, i0);
    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
  }
  store4(i0, sum);
}

// The grid rule, once: a thread per element up to 2048 workgroups, a grid-stride loop beyond.  Every element is summed by one thread
// in the order k = 0 .. splits - 1 whatever the grid, so the result does not depend on it: products and column sums alike take
// this one rule.
int reduce_splits_launch(const float* part, int splits, int64_t mn, float* out, int64_t ldo, int N, float alpha, int accumulate,
                         hipStream_t stream) {
  int64_t blocks = (mn + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  MA_LAUNCH(tn_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, part, splits, mn, out, ldo, N, alpha, accumulate);
  return MA_OK;
}

}  // namespace ma

using namespace ma;

extern "C" int ma_reduce_splits_batch_f32(const ma_reduce_item_t* items, const int32_t* block_item, int32_t n_blocks,
                                          ma_stream_t stream) {
  if (!items || !block_item || n_blocks < 1) return MA_ERR_INVALID_ARG;
  MA_LAUNCH(tn_reduce_batch_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item);
  return MA_OK;
}
