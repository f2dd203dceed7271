// What the TN weight-gradient family (gemm_tn_bf16.hip: 128-wide tiles, gemm_tn8_bf16.hip: 256 x 256 tiles) shares: the layout of a
// partial buffer, the implicit-im2col addressing of the conv2 weight gradient, and the 256-tile entry points the conv2 entry routes to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"

namespace ma {

// A partial buffer: products [splits][rows][No] f32, behind them one partial column-sum vector per split, [splits][rows].
inline int64_t tn_partial_bytes(int64_t splits, int64_t rows, int64_t No) { return splits * rows * (No + 1) * 4; }
inline int64_t tn_cs_offset(int64_t splits, int64_t rows, int64_t No) { return splits * rows * No; }  // in floats

// B as the im2col matrix of a 3x3 stride-2 valid convolution over an NHWC activation (batch, H, Wd, C): row m = (b, ho, wo), column
// (kh, kw, c); B points at the activation.  C is a multiple of the tile width, so the columns of a tile share ONE tap (kh, kw).
struct TnConv {
  int32_t H, Wd, C, Ho, Wo;
  float inv_wo, inv_ho;
};
// tap base of column col = (kh, kw, c): the element of that tap and channel in the window whose top-left pixel is act
__device__ __forceinline__ const uint16_t* tn_conv_tap(const TnConv& cv, const uint16_t* act, int col) {
  const int khw = col / cv.C, kh = khw / 3, kw = khw - 3 * kh;
  return act + ((int64_t)kh * cv.Wd + kw) * cv.C + (col - khw * cv.C);
}
// element offset of contraction row m = (b, ho, wo), m < 2^24: the top-left input pixel of that output pixel
__device__ __forceinline__ int64_t tn_conv_row(const TnConv& cv, int m) {
  const int t = div_small(m, cv.Wo, cv.inv_wo), wo = m - t * cv.Wo;
  const int b = div_small(t, cv.Ho, cv.inv_ho), ho = t - b * cv.Ho;
  return (((int64_t)b * cv.H + 2 * ho) * cv.Wd + 2 * wo) * cv.C;
}

// Number of contraction splits the 256 x 256-tile conv2 weight-gradient kernel uses for (Cout, 9 C) over M rows; 0 = shape not covered.
int tn8_conv_splits(int64_t M, int64_t C, int64_t Cout);
// Partial products [splits][Cout][9 C] at `part`, partial column sums [splits][Cout] at `cs_part` (NULL: none).  MA_OK / MA_ERR_*.
int tn8_conv_launch(const void* dy, int64_t ld_dy, const void* act, int64_t batch, int64_t H, int64_t Wd, int64_t C, int64_t Cout,
                    float* part, float* cs_part, hipStream_t stream);

}  // namespace ma
