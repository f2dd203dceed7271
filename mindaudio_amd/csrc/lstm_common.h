// What the two LSTM schedules share (lstm.hip: one launch per time step of a bidirectional layer; lstm_stack.hip: one launch per
// diagonal of a unidirectional stack): the workgroup geometry, the cell, the packed weights' fragment order, the double-buffered K
// loop and the host-side argument checks.  Where the state and the outputs go, and how partial sums meet in LDS, stays with each file.
//
// Tile.  gates (B, 4H) = A (B, K) . W^T, PyTorch gate order i, f, g, o.  A tile is 16 batch rows x 16 hidden units with ALL FOUR gate
// rows of those units: four 16 x 16 accumulators of v_mfma_f32_16x16x32_bf16, A operand = activations (row = batch), B operand = W
// (column = hidden unit).  The C/D map (column = lane & 15, row = 4 (lane >> 4) + register) puts the four gates of one (batch row,
// hidden unit) into the same lane and register, so the cell needs no lane movement and no memory.  Rows beyond B are never read for
// their own sake (their lanes take row 0's operand; an MFMA row depends on its own A row only) and never stored.
#pragma once
#include "device_common.h"

namespace ma {

constexpr int kLstmThreads = 256;   // 4 waves
constexpr int kLstmSlice = 16;      // hidden units of a workgroup (x 4 gate rows)
constexpr int kLstmRowsPerWg = 64;  // batch rows of a workgroup whose waves own a tile each: 16 per wave

// ---- the cell ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

struct LstmCell {
  float c, h;
};
// gate sums and c_{t-1} in, c_t and h_t out, all float32
__device__ __forceinline__ LstmCell lstm_cell(float gi, float gf, float gg, float go, float c_prev) {
  LstmCell o;
  o.c = lstm_sigmoid(gf) * c_prev + lstm_sigmoid(gi) * tanhf(gg);
  o.h = lstm_sigmoid(go) * tanhf(o.c);
  return o;
}

// The same cell for the training forward, which also keeps the ACTIVATED gates for the backward pass.  c and h are the expressions
// of lstm_cell on the same values, so the two give the same bits (tests/test_lstm_train_gpu.py holds them to that).
struct LstmCellTaped {
  float i, f, g, o, c, h;
};
__device__ __forceinline__ LstmCellTaped lstm_cell_taped(float gi, float gf, float gg, float go, float c_prev) {
  LstmCellTaped o;
  o.i = lstm_sigmoid(gi);
  o.f = lstm_sigmoid(gf);
  o.g = tanhf(gg);
  o.o = lstm_sigmoid(go);
  o.c = o.f * c_prev + o.i * o.g;
  o.h = o.o * tanhf(o.c);
  return o;
}

// The cell backward.  dh = dL/dh_t (the layer's dout plus what came back through W_hh), dc_next = dL/dc_t carried from the step
// that follows in the direction's walk; i, f, g, o, c = the tape of this frame, c_prev = c_{t-1} (0 at the walk's first frame).
// Everything is float32; the gradients of the four pre-activation gate sums leave as they are, the caller rounds them to bf16.
struct LstmCellGrad {
  float di, df, dg, dO, dc_prev;
};
__device__ __forceinline__ LstmCellGrad lstm_cell_bwd(float dh, float dc_next, float i, float f, float g, float o, float c, float c_prev) {
  const float th = tanhf(c);
  const float dc = dh * o * (1.0f - th * th) + dc_next;
  LstmCellGrad r;
  r.dO = dh * th * (o * (1.0f - o));
  r.di = dc * g * (i * (1.0f - i));
  r.dg = dc * i * (1.0f - g * g);
  r.df = dc * c_prev * (f * (1.0f - f));
  r.dc_prev = dc * f;
  return r;
}

// ---- the fragment order -----------------------------------------------------------------------------------------------------------
// A packed weight matrix is [slice of 16 units][k-step of 32][gate][lane][8] bf16: lane l of the wave holds, for hidden unit
// 16 slice + (l & 15), the 8 columns 32 kstep + 8 (l >> 4) .. + 7 of that unit's row of gate g - the B fragment of one MFMA.  The 64
// lanes' fragments of a gate are 1 KiB contiguous, so a wave reads the four gates of a k-step as ONE 4 KiB RUN, straight into
// registers, and the runs of a slice's consecutive k-steps follow each other.  (lstm.hip's two directions are 2 H / 16 slices.)
constexpr int kLstmGateElems = 64 * 8;  // one gate of a run

// lane's fragment of gate 0 in the run of (slice, k-step) of a matrix with nk k-steps per slice; gate g is kLstmGateElems * g further
// and k-step + 1 four gates further.  (Written in this nesting on purpose: the step kernels' register allocation depends on it.)
__device__ __forceinline__ const uint16_t* lstm_gate_run(const uint16_t* w, int nk, int64_t slice, int kstep, int lane) {
  return w + (((slice * nk + kstep) * 4) * 64 + lane) * 8;
}

// the inverse, for the pack kernels: which weights make up fragment i (8 elements) of a matrix with nk k-steps per slice
struct LstmFragment {
  int64_t unit;  // 16 slice + (lane & 15)
  int gate, k;   // first of its 8 columns
};
__device__ __forceinline__ LstmFragment lstm_fragment(int64_t i, int nk) {
  const int lane = (int)(i & 63);
  const int64_t q = i >> 8;  // slice * nk + kstep
  return {q / nk * kLstmSlice + (lane & 15), (int)(i >> 6) & 3, (int)(q % nk) * 32 + 8 * (lane >> 4)};
}
// The backward's order of W_hh (ma_lstm_pack_bwd_f32).  dh (B, H) = dgates (B, 4H) . W_hh contracts over the 4H gate rows
// k = gate * H + unit, and the B operand's column is the hidden unit n that h_{t-1} fed: [slice of 16 units n][k-step of 32 over
// 4H][lane][8] bf16 - lane l holds W_hh[32 kstep + 8 (l >> 4) .. + 7][16 slice + (l & 15)].  One accumulator per tile, so a k-step
// is ONE 1 KiB run and a slice's 4H / 32 runs follow each other (the two directions are 2 H / 16 slices, as above).
__device__ __forceinline__ const uint16_t* lstm_bwd_run(const uint16_t* w, int nk, int64_t slice, int kstep, int lane) {
  return w + ((slice * nk + kstep) * 64 + lane) * 8;
}
// the inverse: fragment i (8 elements) of a matrix with nk = 4H / 32 k-steps per slice holds rows k .. k + 7 of column `unit`
struct LstmBwdFragment {
  int64_t unit;  // 16 slice + (lane & 15), over both directions
  int k;         // first of its 8 gate rows
};
__device__ __host__ __forceinline__ LstmBwdFragment lstm_bwd_fragment(int64_t i, int nk) {
  const int lane = (int)(i & 63);
  const int64_t q = i >> 6;  // slice * nk + kstep
  return {q / nk * 16 + (lane & 15), (int)(q % nk) * 32 + 8 * (lane >> 4)};
}

// columns k .. k + 7 of a float32 weight row of K columns -> one fragment at dst, round to nearest even; columns at or past K are zero
__device__ __forceinline__ void lstm_pack_fragment(const float* row, int k, int K, uint16_t* dst) {
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = k + e < K ? row[k + e] : 0.0f;
  u32x4 o;
  o[0] = pack2_bf16(v[0], v[1]);
  o[1] = pack2_bf16(v[2], v[3]);
  o[2] = pack2_bf16(v[4], v[5]);
  o[3] = pack2_bf16(v[6], v[7]);
  *reinterpret_cast<u32x4*>(dst) = o;
}

// ---- the K loop -------------------------------------------------------------------------------------------------------------------
// KB k-steps of operands for TILES batch tiles: an A fragment per tile and the four gate fragments of W per k-step
template <int KB, int TILES>
struct LstmOperands {
  bf16x8 a[KB][TILES];
  bf16x8 w[KB][4];
};

// acc[tile][gate] = the products of the k-steps [k0, k1) ((k1 - k0) % KB == 0 and k1 > k0: the launcher's choice of KB).
//   run0          lstm_gate_run(.., kstep 0, lane) of the workgroup's slice
//   a_at(t, kk)   where this lane's A fragment of (tile t, k-step kk) is: 16 bytes of row (lane & 15) of the tile, at column
//                 32 kk + 8 (lane >> 4)
//   cell_loads()  the caller's loads of what the cell reads besides the product (projection or bias, c, ...)
// A step's grid is about one workgroup per CU, i.e. one wave per SIMD, so latency is hidden inside the wave or not at all.  Hence the
// issue order: two operand blocks are in registers, and the loads of block i + 1 go out BEFORE the MFMAs of block i, so that the L2
// latency of the weight stream hides behind them; the cell's inputs do not depend on the product, so they are loaded after the first
// block's loads and before the loop, and their latency hides behind all of it.  MFMA order: k-step, then tile, then gate.
// (lstm.hip's lstm_step_ksplit_kernel holds these statements written out, for a measured reason given there: keep the two alike.)
template <int KB, int TILES, class AAt, class CellLoads>
__device__ __forceinline__ void lstm_k_loop(const uint16_t* run0, AAt a_at, int k0, int k1, f32x4 (&acc)[TILES][4], CellLoads cell_loads) {
  auto load = [&](LstmOperands<KB, TILES>& o, int kk0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < KB; ++u) {
#pragma unroll
      for (int g = 0; g < 4; ++g) o.w[u][g] = *reinterpret_cast<const bf16x8*>(run0 + ((int64_t)(kk0 + u) * 4 + g) * kLstmGateElems);
#pragma unroll
      for (int t = 0; t < TILES; ++t) o.a[u][t] = *reinterpret_cast<const bf16x8*>(a_at(t, kk0 + u));
    }
  };
  auto mma = [&](const LstmOperands<KB, TILES>& o) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < KB; ++u)
#pragma unroll
      for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(o.a[u][t], o.w[u][g], acc[t][g], 0, 0, 0);
  };
#pragma unroll
  for (int t = 0; t < TILES; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[t][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  LstmOperands<KB, TILES> cur, nxt;
  load(cur, k0);
  cell_loads();
  for (int kk = k0 + KB; kk < k1; kk += KB) {
    load(nxt, kk);
    mma(cur);
    cur = nxt;
  }
  mma(cur);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

static inline bool lstm_shape_ok(int64_t T, int64_t B, int64_t Kpad, int64_t H) {
  return T >= 1 && B >= 1 && H >= 64 && H % 64 == 0 && H <= 4096 && Kpad >= 64 && Kpad % 64 == 0 && B <= 65535 * (int64_t)kLstmRowsPerWg &&
         B * 4 * H <= 0x7fffffff;
}

// The tape of a training forward (ma_lstm_bidir_train_bf16 writes it, ma_lstm_bidir_bwd_bf16 reads it): act (2, T, 5, B, H) float32,
// per direction and frame the planes i, f, g, o (activated) and c_t; then h (2, T, B, H) bf16, the h_t that was fed back.  A plane
// is (B, H) like c, so the C/D layout stores and loads it the way it does c.
struct LstmTapeLayout {
  int64_t act, h, total;  // byte offsets
};
static inline LstmTapeLayout lstm_tape_layout(int64_t T, int64_t B, int64_t H) {
  LstmTapeLayout t;
  t.act = 0;
  t.h = align256(2 * T * 5 * B * H * 4);
  t.total = t.h + align256(2 * T * B * H * 2);
  return t;
}

// every pointer is 16-byte aligned (the kernels' 16-byte loads and stores start at them)
template <class... P>
static inline bool lstm_aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

}  // namespace ma
