// The one launcher of "sum the splits" (reduce_splits.hip): every host function that adds partial matrices goes through it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ma {

// out[m][n] (+)= alpha * sum over k < splits of part[k][m][n], n < N, mn = rows * N elements per partial, in the order
// k = 0 .. splits - 1 (tn_reduce_kernel).  MA_OK / MA_ERR_LAUNCH.
int reduce_splits_launch(const float* part, int splits, int64_t mn, float* out, int64_t ldo, int N, float alpha, int accumulate,
                         hipStream_t stream);

}  // namespace ma
