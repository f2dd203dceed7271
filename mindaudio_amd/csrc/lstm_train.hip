// Bidirectional LSTM layer, backward through time (the training counterpart of lstm.hip).  Contract: include/mindaudio_amd.h.  The
// tile, the cell backward, the tape layout and the backward fragment order of W_hh are lstm_common.h's; this file holds the schedule.
//
// Schedule.  ma_lstm_bidir_bwd_bf16 issues ONE LAUNCH PER TIME STEP from its host loop, each serving both directions: step s handles
// t = T - 1 - s of the forward direction and t = s of the reverse one (each direction's walk, backwards).  The stream order between the
// launches is the only synchronisation: no workgroup waits for another one (no grid barrier, no flags, no atomics, no graph).
//
// Step kernel.  grid = (H / 16 hidden slices, directions, ceil(B / 64)), 4 waves; wave w owns batch rows 64 z + 16 w .. + 15.
//   1. dh_rec (B, 16) = dgates of the previous launch (B, 4H) . W_hh[:, the slice's 16 units]: the contraction runs over all 4H gate
//      rows, ONE accumulator per batch tile.  K is split over the four waves (4H / 32 is a multiple of 4 for every H % 64 == 0): each
//      runs a quarter of the k-steps for all four tiles, so the workgroup reads its slice of W_hh (4H x 16 bf16) once; the partial
//      sums meet in LDS (12 KB, one workgroup barrier) and wave w adds tile w's four partials in wave order.  There is no form
//      without LDS: it would read the slice once per wave, and no H needs it.
//   2. The cell backward (lstm_cell_bwd) of the wave's tile in the C/D layout, lane-local: dh = dout[t] + dh_rec in float32, the tape's
//      activated gates and c_t, c_{t-1} from the tape's neighbouring frame (0 at the walk's first frame), dc carried in a (2, B, H)
//      float32 buffer that is updated in place, one owner per element.
//   3. The four gate gradients of its units, rounded to bf16, at dgates[dir][t] - the next launch's A operand.
// Rows beyond B read row 0's operand and store nothing.
//
// Rounding points: dgates -> bf16 (round to nearest even), both as the stored result and as the next step's MFMA operand, and W_hh
// -> bf16 in the pack.  dout, dh, dc, the tape and every factor of the cell backward are float32; accumulation is float32.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mindaudio_amd.h"

#include "launch.h"
#include "lstm_common.h"

namespace ma {

struct LstmBwdStep {
  const float* dout;           // (T, B, H)
  const uint16_t* whh;         // backward order, both directions
  const float* act[2];         // the tape's (5, B, H) planes of frame t per direction
  const float* c_prev[2];      // the tape's c plane of the frame before t in the direction's walk; NULL at its first frame
  const uint16_t* dg_prev[2];  // (B, 4H) bf16: dgates of the frame after t in the walk (the previous launch's); NULL in launch 0
  uint16_t* dg[2];             // (B, 4H) bf16: dgates of frame t
  float* dc;                   // (2, B, H): dL/dc carried between launches
  int64_t t[2];                // frame per direction (dout row block)
  int32_t dir0;                // direction of blockIdx.y == 0
  int32_t B, H;
};

constexpr int kLstmBwdPartialFloats = 4 * 3 * 4 * 64;  // [source wave][other tile][register][lane]: 12 KB

// KB = k-steps per operand block (KB x 5 x 16 bytes per lane; two blocks are in flight, as in lstm_k_loop)
template <int KB>
__global__ __launch_bounds__(kLstmThreads) void lstm_bwd_step_kernel(const LstmBwdStep p) {
  __shared__ float part[kLstmBwdPartialFloats];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int z0 = (int)blockIdx.z * kLstmRowsPerWg;
  const int dir = p.dir0 + (int)blockIdx.y, sl = blockIdx.x;
  const int H = p.H, B = p.B;
  const int nk = H / 8, ns = H / kLstmSlice, nkw = nk / 4;  // k-steps of 32 over 4H; a wave's share
  const int64_t plane = (int64_t)B * H;
  const int j = sl * kLstmSlice + (lane & 15);
  const int b0 = z0 + 16 * wave;

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // what the cell backward reads besides the product: issued after the first operand block, consumed after the loop
  float dh[4], gi[4], gf[4], gg[4], go[4], cc[4], cp[4], dcn[4];
  auto cell_loads = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + 4 * (lane >> 4) + r;
      const bool ok = b < B;
      const int64_t e = (int64_t)(ok ? b : 0) * H + j;
      const float* a = p.act[dir] + e;
      dh[r] = ok ? p.dout[p.t[dir] * plane + e] : 0.0f;
      gi[r] = ok ? a[0] : 0.0f;
      gf[r] = ok ? a[plane] : 0.0f;
      gg[r] = ok ? a[2 * plane] : 0.0f;
      go[r] = ok ? a[3 * plane] : 0.0f;
      cc[r] = ok ? a[4 * plane] : 0.0f;
      cp[r] = (ok && p.c_prev[dir]) ? p.c_prev[dir][e] : 0.0f;
      dcn[r] = ok ? p.dc[dir * plane + e] : 0.0f;
    }
  };

  const uint16_t* dgp = p.dg_prev[dir];
  if (dgp) {  // (uniform over the workgroup)
    const uint16_t* ap[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = z0 + 16 * t + (lane & 15);
      ap[t] = dgp + (int64_t)(row < B ? row : 0) * 4 * H + 8 * (lane >> 4) + wave * nkw * 32;
    }
    const uint16_t* wp = lstm_bwd_run(p.whh, nk, (int64_t)dir * ns + sl, wave * nkw, lane);
    struct Operands {
      bf16x8 a[KB][4];
      bf16x8 w[KB];
    };
    auto load = [&](Operands& o, int kk0) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        o.w[u] = *reinterpret_cast<const bf16x8*>(wp + (int64_t)(kk0 + u) * kLstmGateElems);
#pragma unroll
        for (int t = 0; t < 4; ++t) o.a[u][t] = *reinterpret_cast<const bf16x8*>(ap[t] + (kk0 + u) * 32);
      }
    };
    auto mma = [&](const Operands& o) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < KB; ++u)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(o.a[u][t], o.w[u], acc[t], 0, 0, 0);
    };
    Operands cur, nxt;
    load(cur, 0);
    cell_loads();
    for (int kk = KB; kk < nkw; kk += KB) {  // (nkw % KB == 0: the launcher's choice of KB)
      load(nxt, kk);
      mma(cur);
      cur = nxt;
    }
    mma(cur);
  } else {
    cell_loads();
  }

  // tile t's partial from wave s != t sits in slot (t - s - 1) & 3 (0 .. 2) of wave s's block
  f32x4 own = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t == wave) {
      own = acc[t];
    } else {
      float* dst = part + ((wave * 3 + ((t - wave - 1) & 3)) * 4) * 64 + lane;
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[r * 64] = acc[t][r];
    }
  }
  __syncthreads();  // (within the workgroup; every wave arrives: nothing returns before this line)
  f32x4 tot = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {  // wave order = K order
    if (s == wave) {
      tot += own;
    } else {
      const float* src = part + ((s * 3 + ((wave - s - 1) & 3)) * 4) * 64 + lane;
#pragma unroll
      for (int r = 0; r < 4; ++r) tot[r] += src[r * 64];
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + 4 * (lane >> 4) + r;
    if (b >= B) continue;
    const LstmCellGrad g = lstm_cell_bwd(dh[r] + tot[r], dcn[r], gi[r], gf[r], gg[r], go[r], cc[r], cp[r]);
    p.dc[dir * plane + (int64_t)b * H + j] = g.dc_prev;
    uint16_t* o = p.dg[dir] + (int64_t)b * 4 * H + j;
    o[0] = f2bf(g.di);
    o[H] = f2bf(g.df);
    o[2 * H] = f2bf(g.dg);
    o[3 * H] = f2bf(g.dO);
  }
}

// W_hh (2, 4H, H) f32 -> the backward fragment order, the directions as 2 H / 16 slices
__global__ __launch_bounds__(256) void lstm_pack_bwd_kernel(const float* __restrict__ w, int H, int64_t groups, uint16_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one 8-element fragment
  if (i >= groups) return;
  const LstmBwdFragment f = lstm_bwd_fragment(i, H / 8);
  const int64_t dir = f.unit / H, n = f.unit % H;
  const float* col = w + (dir * 4 * H + f.k) * H + n;  // rows k .. k + 7 of column n
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack2_bf16(col[(int64_t)(2 * e) * H], col[(int64_t)(2 * e + 1) * H]);
  *reinterpret_cast<u32x4*>(out + i * 8) = o;
}

}  // namespace ma

using namespace ma;

extern "C" {

int ma_lstm_pack_bwd_f32(const float* w_hh, int32_t H, void* whh_bwd_packed, ma_stream_t stream) {
  if (!w_hh || !whh_bwd_packed || H < 1) return MA_ERR_INVALID_ARG;
  if (!lstm_shape_ok(1, 1, 64, H)) return MA_ERR_UNSUPPORTED;
  if (!lstm_aligned16(whh_bwd_packed)) return MA_ERR_INVALID_ARG;
  const int64_t groups = 2 * 4 * (int64_t)H * H / 8;
  MA_LAUNCH(lstm_pack_bwd_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_hh, H, groups,
            reinterpret_cast<uint16_t*>(whh_bwd_packed));
  return MA_OK;
}

int64_t ma_lstm_bwd_workspace_bytes(int64_t B, int32_t H) {
  if (B < 1 || H < 1) return MA_ERR_INVALID_ARG;
  if (!lstm_shape_ok(1, B, 64, H)) return MA_ERR_UNSUPPORTED;
  return align256(2 * B * H * 4);
}

int ma_lstm_bidir_bwd_bf16(const float* dout, int64_t T, int64_t B, int32_t H, const void* tape, int64_t tape_bytes,
                           const void* whh_bwd_packed, int32_t dir_mask, void* dgates, void* workspace, int64_t workspace_bytes,
                           ma_stream_t stream) {
  if (!dout || !tape || !whh_bwd_packed || !dgates || !workspace || T < 1 || B < 1 || H < 1 || dir_mask < 1 || dir_mask > 3)
    return MA_ERR_INVALID_ARG;
  if (!lstm_shape_ok(T, B, 64, H)) return MA_ERR_UNSUPPORTED;
  if (!lstm_aligned16(dout, tape, whh_bwd_packed, dgates, workspace)) return MA_ERR_INVALID_ARG;
  const LstmTapeLayout tl = lstm_tape_layout(T, B, H);
  if (tape_bytes < tl.total || workspace_bytes < align256(2 * B * H * 4)) return MA_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t bh = B * H, g4 = 4 * (int64_t)H;
  const float* act = reinterpret_cast<const float*>(reinterpret_cast<const char*>(tape) + tl.act);
  uint16_t* dg = reinterpret_cast<uint16_t*>(dgates);
  float* dc = reinterpret_cast<float*>(workspace);
  if (ensure_init() != MA_OK) return MA_ERR_LAUNCH;
  if (hipMemsetAsync(dc, 0, (size_t)(2 * bh * 4), st) != hipSuccess) return MA_ERR_LAUNCH;
  for (int d = 0; d < 2; ++d)  // a direction that did not run has no gradient
    if (!(dir_mask & (1 << d)) && hipMemsetAsync(dg + d * T * B * g4, 0, (size_t)(T * B * g4 * 2), st) != hipSuccess) return MA_ERR_LAUNCH;

  const dim3 grid((unsigned)(H / kLstmSlice), dir_mask == 3 ? 2u : 1u, (unsigned)((B + kLstmRowsPerWg - 1) / kLstmRowsPerWg));
  for (int64_t s = 0; s < T; ++s) {
    LstmBwdStep p;
    p.dout = dout;
    p.whh = reinterpret_cast<const uint16_t*>(whh_bwd_packed);
    p.dc = dc;
    p.dir0 = dir_mask == 2 ? 1 : 0;
    p.B = (int32_t)B;
    p.H = H;
    p.t[0] = T - 1 - s;
    p.t[1] = s;
    // the frame before t in the direction's forward walk (c_{t-1}) and the one after it (whose dgates came with the last launch)
    const int64_t before[2] = {p.t[0] - 1, p.t[1] + 1}, after[2] = {p.t[0] + 1, p.t[1] - 1};
    for (int d = 0; d < 2; ++d) {
      p.act[d] = act + (d * T + p.t[d]) * 5 * bh;
      p.c_prev[d] = (before[d] >= 0 && before[d] < T) ? act + (d * T + before[d]) * 5 * bh + 4 * bh : nullptr;
      p.dg_prev[d] = s > 0 ? dg + (d * T + after[d]) * B * g4 : nullptr;
      p.dg[d] = dg + (d * T + p.t[d]) * B * g4;
    }
    if ((H / 32) % 4 == 0) MA_LAUNCH(lstm_bwd_step_kernel<4>, grid, dim3(kLstmThreads), 0, st, p);
    else MA_LAUNCH(lstm_bwd_step_kernel<2>, grid, dim3(kLstmThreads), 0, st, p);
  }
  return MA_OK;
}

}  // extern "C"
