// Conv2dSubsampling4's two convolutions in ONE launch (mindaudio/models/layers/subsampling.py:40-45 with GlobalCMVN,
// layers/cmvn.py:33-35, in front):
//
//     act1[b, h, w, c] = relu(b1[c] + sum_{i, j < 3} W1[c, i, j] xn[b, 2 h + i, 2 w + j]),   xn = (x - mean) istd
//     out[b, ho, wo, n] = relu(b2[n] + sum_{kh, kw, c} act1[b, 2 ho + kh, 2 wo + kw, c] W2[n, kh, kw, c])
//
// Until round 4 these were two kernels per utterance group: subsample_conv1_c256_kernel wrote act1 (637 MB of bf16 at the north-star
// batch) and conv2_packed_kernel read it straight back through a 3-stage LDS ring of im2col copies.  act1 is 9 multiply-adds per
// element of a ONE-channel input, so here it never leaves the CU.  A workgroup = 8 waves = 4 CONSUMERS + 4 PRODUCERS, one per CU:
//   * it owns 128 consecutive output positions (ho, wo) of one utterance x all 256 output channels; consumer wave w owns channels
//     64 w .. 64 w + 63 against the 128 positions (32 accumulator tiles, as conv2_packed.hip), its W2 fragments stream L2 -> registers
//     from a fragment-ordered packed copy through an 8-slot ring two taps ahead (counted vmcnt, never drained inside the launch);
//   * the <= 35 CMVN-normalised input rows the tile depends on are staged in LDS once (11 KB), and from them the im2col view X of
//     conv1: per act1 position (<= 17 x 39 of them) the 9 taps as bf16 (hi, hi, lo) triples - see below;
//   * the contraction runs over 8 chunks of 32 act1 channels.  The producers BUILD the act1 patch of chunk k + 1 - positions x 32
//     channels, bf16, 80-byte position pitch, into the other of two LDS buffers - while the consumers CONTRACT patch k: the im2col
//     view of conv2 is pure ADDRESSING into the patch - the A fragment of output position (ho, wo), tap (kh, kw) is the 64 bytes at
//     patch[2 (ho - ho0) + kh][2 wo + kw] - so a consumer lane keeps one LDS address per row tile and the tap is an immediate offset.
//     No staging copies, no LDS-DMA ring, one barrier per chunk (= per 288 MFMAs per wave; conv2_packed has one barrier + one counted
//     wait per 64).  With the 80-byte pitch the 16 lanes of a ds_read_b128 group (stride 2 positions = 160 bytes) fall on 16 distinct
//     16-byte slots;
//   * conv1 itself runs on the matrix pipe.  (The first version of this kernel built the patch with the stand-alone kernel's float32
//     FMA chain: 72 v_fmac per position and wave - 9 000 cycles per patch against 5 700 for the contraction it feeds,
//     profiles/r05_subsample_fused_timeline.txt.)  A float32 product x w is split as x = xh + xl, w = wh + wl (bf16 head + bf16 tail,
//     both exact in float32) and computed as xh wh + xh wl + xl wh: 27 <= 32 k-values, ONE v_mfma_f32_16x16x32_bf16 per
//     16 positions x 16 channels with the bias as the C operand.  The neglected xl wl term and the tails' own rounding are 2^-16 of a
//     product - 1.5e-5 relative in front of a bf16 rounding of 3.9e-3: act1 differs from the stand-alone kernel's in the last bf16
//     bit of about one element in 200 (tests/test_conformer_ops_gpu.py::test_subsample_fused bounds it).  84 MFMAs per chunk instead
//     of 48 000 FMAs.
// Removed with it: the 637 MB write + read, the utterance grouping through the Infinity Cache and three launches per step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/mindaudio_amd.h"

#include "device_common.h"
#include "launch.h"

namespace ma {

constexpr int kSfRows = 128, kSfC = 256, kSfThreads = 512;  // 4 consumer (conv2) waves + 4 producer (conv1) waves
constexpr int kSfIdim = 80, kSfF1 = 39, kSfF2 = 19;         // feature axis: 80 -> 39 -> 19
constexpr int kSfNhoMax = 8;                                // output rows a 128-position tile can touch
constexpr int kSfH1Max = 2 * kSfNhoMax + 1;                 // act1 rows of the patch
constexpr int kSfInMax = 2 * kSfH1Max + 1;                  // input rows
constexpr int kSfPosMax = 672;                              // 17 x 39 = 663 patch positions, in whole 16-position tiles
constexpr int kSfPitch = 80;                                // bytes per patch position: 32 channels bf16 + 16 of padding
constexpr int kSfChunks = 8, kSfTaps = 9;
constexpr int kSfW2Bytes = kSfC * 9 * kSfC * 2;             // packed W2; the packed W1 fragments (16 KiB) follow it
// LDS: input rows | X (conv1's im2col, 64 B per position) | patch buffer 0 | patch buffer 1
constexpr int kSfOffX = 11264;                              // input rows: 35 x 80 x 4 = 11 200 B
constexpr int kSfOffPatch = kSfOffX + kSfPosMax * 64;
constexpr int kSfPatchBytes = kSfPosMax * kSfPitch;         // 53 760
constexpr int kSfLds = kSfOffPatch + 2 * kSfPatchBytes;     // 161 792 B: one workgroup per CU
constexpr int kSfOutPitch = 144;                            // epilogue staging: 128 B of a wave's 64 channels + 16 of padding
static_assert(kSfInMax * kSfIdim <= 6 * kSfThreads && kSfPosMax <= 2 * kSfThreads && kSfLds <= 163840, "tile geometry");
static_assert(4 * kSfRows * kSfOutPitch <= kSfOffPatch + kSfPatchBytes, "epilogue staging must not reach patch buffer 1");
static_assert(4 * (kSfRows / 2) * kSfOutPitch <= kSfPatchBytes, "the walking kernel stages half a tile inside patch buffer 1");
static_assert(kSfInMax * kSfIdim <= 12 * (kSfThreads / 2), "the producer waves alone stage the next tile's input rows");

struct SubsampleFusedParams {
  const float* x;  // (B, T, 80) float32, any strides
  int64_t sb, st, sf;
  const float *mean, *istd;  // CMVN, may be NULL
  const char* packed;        // [W2: wave 4][chunk 8][tap 9][tile 4][lane 64] x 16 B | [W1: chunk 8][tile 2][lane 64] x 16 B
  const float* b1;
  const float* b2;
  uint16_t* out;             // (B, Ho, Wo, 256) bf16
  int32_t Ho, tiles_per_utt;
  int32_t ntiles;            // batch * tiles_per_utt
};

// What the code of one tile depends on: tile t = utterance b, output positions p0 .. p0 + np - 1 of it.
struct SfTile {
  int b, p0, np, ho0, nin, npatch;
};

__device__ __forceinline__ SfTile sf_tile(const SubsampleFusedParams& p, int t) {
  SfTile g;
  g.b = t / p.tiles_per_utt;
  g.p0 = (t - g.b * p.tiles_per_utt) * kSfRows;
  g.np = min(kSfRows, p.Ho * kSfF2 - g.p0);
  g.ho0 = g.p0 / kSfF2;
  const int nho = (g.p0 + g.np - 1) / kSfF2 - g.ho0 + 1;
  const int nh1 = 2 * nho + 1;
  g.nin = 2 * nh1 + 1;
  g.npatch = nh1 * kSfF1;
  return g;
}

// A thread's share of a tile's input rows between their request and their LDS write (J = 6 with all 512 threads, 12 with the 256
// of the producer waves).
template <int J_>
struct SfRowRegs {
  static constexpr int J = J_;
  float v[J_], mu[J_], is[J_];
  int dst[J_];
};

// x rounded to bf16 (nearest even), as a float
__device__ __forceinline__ float sf_head(float x) { return __uint_as_float(pack2_bf16(x, 0.0f) << 16); }

// The 32 k-values of one conv1 operand row from its 9 float32 taps v: X = (head, head, tail), W = (head, tail, head) at
// k = 0..8 | 9..17 | 18..26 (27..31 zero)  ->  sum_k X[k] W[k] = xh wh + xh wl + xl wh per tap.
template <bool IS_W>
__device__ __forceinline__ void sf_split_row(const float (&v)[9], uint32_t (&d)[16]) {
  float h[9], l[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    h[t] = sf_head(v[t]);
    l[t] = v[t] - h[t];  // exact; its own bf16 rounding (in the packing below) is the 2^-16 term of the header
  }
  float k[32];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    k[t] = h[t];
    k[9 + t] = IS_W ? l[t] : h[t];
    k[18 + t] = IS_W ? h[t] : l[t];
  }
#pragma unroll
  for (int t = 27; t < 32; ++t) k[t] = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) d[j] = pack2_bf16(k[2 * j], k[2 * j + 1]);
}

// W2 item (wave w, chunk cc, tap, tile jt): lane (i, g) holds W2[64 w + 16 jt + i][tap][32 cc + 8 g .. + 8].
// W1 item (chunk cc, tile t): lane (i, g) holds k-values 8 g .. 8 g + 7 of channel 32 cc + 16 t + i.
__global__ void subsample_fused_pack_kernel(const uint16_t* __restrict__ w2, const float* __restrict__ w1, uint4* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // 4 * 72 * 4 * 64 = 73728 pieces of W2, then 16 * 64 = 1024 of W1
  constexpr int kN2 = 4 * kSfChunks * kSfTaps * 4 * 64;
  if (idx < kN2) {
    const int lane = idx & 63, jt = (idx >> 6) & 3, ft = (idx >> 8) % (kSfChunks * kSfTaps), wv = (idx >> 8) / (kSfChunks * kSfTaps);
    const int cc = ft / kSfTaps, tap = ft - cc * kSfTaps;
    const int n = 64 * wv + 16 * jt + (lane & 15);
    out[idx] = *reinterpret_cast<const uint4*>(w2 + (int64_t)n * (9 * kSfC) + tap * kSfC + 32 * cc + 8 * (lane >> 4));
  } else if (idx < kN2 + 16 * 64) {
    const int j = idx - kN2, lane = j & 63, item = j >> 6;
    const int ch = 16 * item + (lane & 15), g = lane >> 4;
    float v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) v[t] = w1[ch * 9 + t];
    uint32_t d[16];
    sf_split_row<true>(v, d);
    out[idx] = g == 0 ? make_uint4(d[0], d[1], d[2], d[3]) : g == 1 ? make_uint4(d[4], d[5], d[6], d[7])
             : g == 2 ? make_uint4(d[8], d[9], d[10], d[11]) : make_uint4(d[12], d[13], d[14], d[15]);
  }
}

// wave priorities of the two roles (development A/B: -DSF_PRIO_C=x -DSF_PRIO_P=y)
#ifndef SF_PRIO_C
#define SF_PRIO_C 1
#endif
#ifndef SF_PRIO_P
#define SF_PRIO_P 0
#endif
// Phase stamps for tools/subsample_timeline.py (compiled in only with -DMA_SF_PROF; the shipped library has none of it): consumer wave 0
// and producer wave 4 of three workgroups (the first, the middle one, the sixth from the end of the grid) write s_memtime (shader
// clock) at their phase boundaries, for four tiles of the workgroup's walk: its first, the middle one, the one after that, its last.
// The stamps are absolute, so the tool can subtract across tiles and roles.  Each stamp is stored at once: kept in registers until
// the tile's end, 32 of them made the compiler spill (and so did a branch around the store), and a spilled W2 ring register whose
// load is still in flight is a stale copy there and a late write here - the instrumented build must stay at .vgpr_spill_count 0
// like the shipped one.
#ifdef MA_SF_PROF
__device__ unsigned long long g_sf_prof[2 * 3 * 4 * 32 + 32];  // (+ 32: where every wave that is not sampled stamps)
__device__ __forceinline__ int sf_prof_slot(int wave, int i, int ntiles) {
  const int role = wave == 0 ? 0 : wave == 4 ? 1 : -1;
  const int wg = blockIdx.x == 0 ? 0 : blockIdx.x == gridDim.x / 2 ? 1 : blockIdx.x + 6 == gridDim.x ? 2 : -1;
  const int cnt = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int ts = i == 0 ? 0 : i == cnt - 1 ? 3 : i == cnt / 2 ? 1 : i == cnt / 2 + 1 ? 2 : -1;
  return role < 0 || wg < 0 || ts < 0 ? 2 * 3 * 4 * 32 : ((role * 3 + wg) * 4 + ts) * 32;
}
#define SF_STAMP(k)                                                        \
  do {                                                                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();            \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
    g_sf_prof[sf_slot + (k)] = t_; /* no branch: all lanes, one address */ \
  } while (0)
#define SF_NEXT_TILE() (sf_slot = sf_prof_slot(wave, ++sf_i, p.ntiles))
#else
#define SF_STAMP(k) do { } while (0)
#define SF_NEXT_TILE() do { } while (0)
#endif

// WALK = false: one tile per workgroup (grid = tiles), the form this kernel had before it walked - kept as the reference the walking
// form is compared with bit for bit, and for A/B (MINDAUDIO_AMD_SUBSAMPLE=tile).
// WALK = true: a workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (a static list: no counter in memory, the trip
// count is the same for its eight waves, so every barrier below is reached by all of them equally often; tiles may cross utterances).
// Its first tile starts as above, with all eight waves in the prologue.  From then on the prologue of tile n + 1 - 14 000 cycles in
// which the matrix pipe has nothing to do - is the PRODUCERS' work while the consumers finish tile n:
//
//     barrier   consumers                        producers
//     B5        chunk 5 (buffer 1)               request the rows of n + 1 (the rows region is free once X of n is built); build patch 6
//     B6        chunk 6 (patch buffer 0)         build patch 7 (X -> buffer 1); write the rows of n + 1 (CMVN applied)
//     B7        chunk 7 (buffer 1)               build X of n + 1 (X is free: patch 7 is built)
//     Bx        epilogue (staged in buffer 1)    build patch 0 of n + 1 into buffer 0 (free since B7), four waves
//     Bj        chunk 0 of n + 1                 build patch 1 of n + 1 into buffer 1 ...
//
// So that nothing of tile n lies where tile n + 1 is being built, the epilogue's wave-private staging strips are in patch buffer 1,
// which is dead after chunk 7 - for EVERY consumer only after Bx, the one barrier this form adds to a tile (the one-tile form stages
// in rows / X / buffer 0, which chunk 7 does not read, and needs none).  Half a tile fits there, so the tile leaves in two half passes
// (row tiles 0-3, then 4-7) through the same strip; LDS operations of one wave execute in order, so no barrier lies between them.
// The W2 ring wraps from tap 71 of tile n to tap 0 of tile n + 1 and stays in flight across the epilogue and Bj: vmcnt(0) only after
// the last tile.  (The epilogue's stores are younger than the wrapped loads and loads return in order, so the counted waits of the
// next chunk 0 still cover the fragments they name.)
template <bool WALK>
__global__ __launch_bounds__(kSfThreads, 2) void subsample_fused_kernel(const SubsampleFusedParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef MA_SF_PROF
  int sf_i = 0, sf_slot = sf_prof_slot(wave, 0, p.ntiles);
#endif
  SF_STAMP(0);
  const int npos = p.Ho * kSfF2;                 // output positions of one utterance
  int t = blockIdx.x;
  const int tstep = gridDim.x;
  SfTile g = sf_tile(p, t);
  float* rows = reinterpret_cast<float*>(smem);
  char* xim = smem + kSfOffX;
  char* patch = smem + kSfOffPatch;

  // ---- a tile's input rows, CMVN applied: rows[r][f] = xn[b, 4 ho0 + r, f], thread tt of nthr.  All loads are requested before the
  // first store (as a load -> store loop the six round trips to HBM ran one after the other: 5 900 cycles) ----------------------------
  auto rows_request = [&](const SfTile& q, int tt, int nthr, auto& r) __attribute__((always_inline)) {
    constexpr int J = std::remove_reference_t<decltype(r)>::J;
    const float* xb = p.x + (int64_t)q.b * p.sb + (int64_t)(4 * q.ho0) * p.st;
    const bool tfast = p.st <= p.sf;  // time is the fast axis of the view (fbank's (B, n_mels, T) output): walk it first
    const int n = q.nin * kSfIdim;
    // every address first, then nothing but loads: mixed with the index arithmetic, the compiler's register reuse put a wait for
    // ALL of them in front of whatever came next (in the walking form: patch 7)
    int64_t off[J];
    int f[J];
    const int magic = (1 << 20) / q.nin + 1;  // i / nin = (i magic) >> 20 for i < 4096, nin <= 35 (exact while i nin < 2^20)
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int i = min(tt + nthr * j, n - 1);
      f[j] = tfast ? (i * magic) >> 20 : i % kSfIdim;
      const int rr = tfast ? i - f[j] * q.nin : i / kSfIdim;
      r.dst[j] = rr * kSfIdim + f[j];
      off[j] = rr * p.st + f[j] * p.sf;
    }
    __builtin_amdgcn_sched_barrier(0);
    // (without CMVN the same loads from b1, unused: one straight run of loads either way, so that the compiler's own wait counts
    // downstream are exact and not the worst case of two paths)
    const float *mp = p.mean ? p.mean : p.b1, *ip = p.mean ? p.istd : p.b1;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      r.v[j] = xb[off[j]];
      r.mu[j] = mp[f[j]];
      r.is[j] = ip[f[j]];
    }
  };
  auto rows_write = [&](const SfTile& q, int tt, int nthr, const auto& r) __attribute__((always_inline)) {
    constexpr int J = std::remove_reference_t<decltype(r)>::J;
    const int n = q.nin * kSfIdim;
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (tt + nthr * j < n) rows[r.dst[j]] = p.mean ? (r.v[j] - r.mu[j]) * r.is[j] : r.v[j];
  };
  // ---- X: per patch position (h, w) the 9 taps rows[2 h + i][2 w + j] as (head, head, tail) bf16 triples, 64 bytes --------------------
  auto build_x = [&](const SfTile& q, int tt, auto nthrc) __attribute__((always_inline)) {
    constexpr int NTHR = decltype(nthrc)::value;
#pragma unroll
    for (int j = 0; j < (kSfPosMax + NTHR - 1) / NTHR; ++j) {
      const int pos = tt + NTHR * j;
      if (pos < kSfPosMax) {
        uint32_t d[16];
        if (pos < q.npatch) {
          const int h = pos / kSfF1, w = pos - h * kSfF1;
          const float* in = rows + (2 * h) * kSfIdim + 2 * w;
          float v[9];
#pragma unroll
          for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) v[kh * 3 + kw] = in[kh * kSfIdim + kw];
          sf_split_row<false>(v, d);
        } else {
#pragma unroll
          for (int q4 = 0; q4 < 16; ++q4) d[q4] = 0u;  // positions past the patch: finite operands for the (unused) tail of the last tile
        }
        uint4* xo = reinterpret_cast<uint4*>(xim + pos * 64);
        xo[0] = make_uint4(d[0], d[1], d[2], d[3]);
        xo[1] = make_uint4(d[4], d[5], d[6], d[7]);
        xo[2] = make_uint4(d[8], d[9], d[10], d[11]);
        xo[3] = make_uint4(d[12], d[13], d[14], d[15]);
      }
    }
  };
  // ---- one chunk's act1 patch on the matrix pipe: D[channel][position] = W1frag . Xfrag + b1; producer pw of nprod takes the
  // 16-position tiles pw, pw + nprod, ... for both 16-channel tiles of the chunk ---------------------------------------------------------
  const int ci = lane & 15, gi = lane >> 4;
  struct PatchOps {  // a chunk's W1 fragments and bias, requested apart from their use so that other loads can be queued behind them
    uint4 wa, wb;
    float4 ba, bb;
  };
  auto patch_operands = [&](int cc) __attribute__((always_inline)) {
    const uint4* w1f = reinterpret_cast<const uint4*>(p.packed + kSfW2Bytes) + (2 * cc) * 64 + lane;
    PatchOps o;
    o.wa = w1f[0];
    o.wb = w1f[64];
    o.ba = *reinterpret_cast<const float4*>(p.b1 + 32 * cc + 4 * gi);
    o.bb = *reinterpret_cast<const float4*>(p.b1 + 32 * cc + 16 + 4 * gi);
    return o;
  };
  auto build_patch_with = [&](const PatchOps& w, int npatch, int cc, int pw, int nprod) __attribute__((always_inline)) {
    const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&w.wa), a1 = *reinterpret_cast<const bf16x8*>(&w.wb);
    const f32x4 c0 = {w.ba.x, w.ba.y, w.ba.z, w.ba.w}, c1 = {w.bb.x, w.bb.y, w.bb.z, w.bb.w};
    const char* xsrc = xim + ci * 64 + gi * 16;
    char* dst = patch + (cc & 1) * kSfPatchBytes + ci * kSfPitch + gi * 8;
    const int ntile = (npatch + 15) >> 4;
    auto put = [&](int pt, const f32x4& d0, const f32x4& d1) __attribute__((always_inline)) {
      char* o = dst + pt * (16 * kSfPitch);
      *reinterpret_cast<uint2*>(o) = make_uint2(pack2_bf16(fmaxf(d0[0], 0.f), fmaxf(d0[1], 0.f)), pack2_bf16(fmaxf(d0[2], 0.f), fmaxf(d0[3], 0.f)));
      *reinterpret_cast<uint2*>(o + 32) = make_uint2(pack2_bf16(fmaxf(d1[0], 0.f), fmaxf(d1[1], 0.f)), pack2_bf16(fmaxf(d1[2], 0.f), fmaxf(d1[3], 0.f)));
    };
    // two position tiles per trip: a trip is one chain LDS read -> MFMA -> pack -> LDS write; two independent chains shorten the
    // prologue's patch 0 (2 270 -> 2 000 ticks) but not a patch built beside contracting consumers (5 000 - 5 600 either way)
    for (int pt = pw; pt < ntile; pt += 2 * nprod) {
      const int pt1 = pt + nprod;
      const bool two = pt1 < ntile;
      const uint4 xr0 = *reinterpret_cast<const uint4*>(xsrc + pt * (16 * 64));
      const uint4 xr1 = *reinterpret_cast<const uint4*>(xsrc + (two ? pt1 : pt) * (16 * 64));
      const bf16x8 xf0 = *reinterpret_cast<const bf16x8*>(&xr0), xf1 = *reinterpret_cast<const bf16x8*>(&xr1);
      const f32x4 d00 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, xf0, c0, 0, 0, 0);
      const f32x4 d01 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, xf0, c1, 0, 0, 0);
      const f32x4 d10 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, xf1, c0, 0, 0, 0);
      const f32x4 d11 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, xf1, c1, 0, 0, 0);
      put(pt, d00, d01);
      if (two) put(pt1, d10, d11);
    }
  };
  auto build_patch = [&](int npatch, int cc, int pw, int nprod) __attribute__((always_inline)) {
    build_patch_with(patch_operands(cc), npatch, cc, pw, nprod);
  };

  // ---- the workgroup's first tile: rows, X and patch 0 by all 8 waves ------------------------------------------------------------------
  {
    SfRowRegs<6> r;
    rows_request(g, tid, kSfThreads, r);
    rows_write(g, tid, kSfThreads, r);
  }
  __syncthreads();
  SF_STAMP(1);
  build_x(g, tid, std::integral_constant<int, kSfThreads>{});
  __syncthreads();
  SF_STAMP(2);
  build_patch(g.npatch, 0, wave, 8);
  SF_STAMP(3);

  if (wave >= 4) {
    // ================= producer waves: patch k + 1 is built while the consumers contract patch k; under the tile's last chunk and
    // epilogue, everything the next tile needs before its chunk 0 =====================================================================
#if SF_PRIO_P
    __builtin_amdgcn_s_setprio(SF_PRIO_P);
#endif
    const int ptid = tid - kSfThreads / 2;
    for (;;) {
      const int tn = t + tstep;
      const bool more = WALK && tn < p.ntiles;
#pragma unroll 1
      for (int k = 0; k + 3 < kSfChunks; ++k) {
        __syncthreads();  // B0 (= Bj of the tile before) .. B4  (the compiler's fence in front of it retires this wave's LDS writes:
                          // patch k is complete)
        SF_STAMP(4 + 2 * k);
        build_patch(g.npatch, k + 1, wave - 4, 4);
        SF_STAMP(5 + 2 * k);
      }
      __syncthreads();  // B5
      SF_STAMP(14);
      SfTile gn = g;
      SfRowRegs<12> r;
      const PatchOps w6 = patch_operands(kSfChunks - 2);  // in front of the row requests: patch 6 must not wait for those
      if (more) {  // the rows region has been free since this tile's X was built; the requests fly under patches 6 and 7
        gn = sf_tile(p, tn);
        rows_request(gn, ptid, kSfThreads / 2, r);
        SF_STAMP(22);
        build_patch_with(w6, g.npatch, kSfChunks - 2, wave - 4, 4);
      } else {  // (its own copy of the loop: joined with the arm above, the loop would wait for that arm's row loads)
        build_patch_with(w6, g.npatch, kSfChunks - 2, wave - 4, 4);
      }
      SF_STAMP(15);
      __syncthreads();  // B6
      SF_STAMP(16);
      build_patch(g.npatch, kSfChunks - 1, wave - 4, 4);
      SF_STAMP(17);
      if (more) {
        rows_write(gn, ptid, kSfThreads / 2, r);
        SF_STAMP(23);
      }
      __syncthreads();  // B7: patch 7 and the next rows are complete
      SF_STAMP(20);
      if constexpr (!WALK) {
        return;
      } else {
        if (more) {
          build_x(gn, ptid, std::integral_constant<int, kSfThreads / 2>{});
          SF_STAMP(24);
        }
        __syncthreads();  // Bx: the next X is complete; every consumer is past chunk 7
        SF_STAMP(27);
        if (more) {
          build_patch(gn.npatch, 0, wave - 4, 4);  // buffer 0: the consumers left it at B7
          SF_STAMP(25);
        }
        if (!more) return;
        g = gn;
        t = tn;
        SF_NEXT_TILE();
        SF_STAMP(0);
      }
    }
  }

  // ================= consumer waves: wave w -> output channels 64 w .. 64 w + 63 against the tile's 128 positions ================
#if SF_PRIO_C
  __builtin_amdgcn_s_setprio(SF_PRIO_C);
#endif
  const int c = ci, gq = gi;
  uint32_t a_addr[8];
  // W2 fragments: SGPR base of the flat tap + lane offset; ring of 8 = two taps.  Past the last tap of a tile: the one-tile form
  // repeats tap 71 (duplicates, drained at the end), the walking form wraps to taps 0 and 1 - of the next tile.
  const uint32_t voff = lane * 16 + 2048;
  const char* wbase = p.packed + (int64_t)wave * (kSfChunks * kSfTaps) * 4096;
#define SF_LOAD(dst, ft, jt)                                                                                          \
  do {                                                                                                                \
    const int ft_ = (ft) < kSfChunks * kSfTaps ? (ft) : WALK ? (ft) - kSfChunks * kSfTaps : kSfChunks * kSfTaps - 1;  \
    const char* cb_ = wbase + (int64_t)ft_ * 4096;                                                                    \
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(cb_), "n"(((jt) - 2) * 1024) \
                 : "memory");                                                                                         \
  } while (0)
  bf16x8 ring[8];
  f32x4 acc[4][8];
  bf16x8 af[2][8];
#define SF_LDS(dst, s_, imm_) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(a_addr[s_]), "n"(imm_) : "memory")
#define SF_LDS8(buf_, imm_)                                                                                   \
  SF_LDS(af[buf_][0], 0, imm_); SF_LDS(af[buf_][1], 1, imm_); SF_LDS(af[buf_][2], 2, imm_); SF_LDS(af[buf_][3], 3, imm_); \
  SF_LDS(af[buf_][4], 4, imm_); SF_LDS(af[buf_][5], 5, imm_); SF_LDS(af[buf_][6], 6, imm_); SF_LDS(af[buf_][7], 7, imm_)
  // ---- one tap of one chunk: 8 A fragments x 4 W2 fragments = 32 MFMAs.  BUF = patch buffer (chunk parity), PAR = parity of the
  // flat tap index (register halves of the A double buffer and of the W2 ring) -------------------------------------------------------
  auto tap_step = [&](auto tapc, auto parc, auto bufc, int ft) __attribute__((always_inline)) {
    constexpr int TAP = decltype(tapc)::value, PAR = decltype(parc)::value, BUF = decltype(bufc)::value;
    constexpr int IMM = BUF * kSfPatchBytes + ((TAP / 3) * kSfF1 + (TAP % 3)) * kSfPitch;
    constexpr int NTAP = TAP + 1;
    constexpr int IMM_N = BUF * kSfPatchBytes + ((NTAP / 3) * kSfF1 + (NTAP % 3)) * kSfPitch;
    if constexpr (TAP == 0) { SF_LDS8(PAR, IMM); }
    if constexpr (TAP < kSfTaps - 1) {
      SF_LDS8(PAR ^ 1, IMM_N);
      asm volatile("s_waitcnt lgkmcnt(8)"
                   : "+v"(af[PAR][0]), "+v"(af[PAR][1]), "+v"(af[PAR][2]), "+v"(af[PAR][3]), "+v"(af[PAR][4]), "+v"(af[PAR][5]),
                     "+v"(af[PAR][6]), "+v"(af[PAR][7])::"memory");
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(af[PAR][0]), "+v"(af[PAR][1]), "+v"(af[PAR][2]), "+v"(af[PAR][3]), "+v"(af[PAR][4]), "+v"(af[PAR][5]),
                     "+v"(af[PAR][6]), "+v"(af[PAR][7])::"memory");
    }
    static_for<4>([&](auto tc) __attribute__((always_inline)) {
      constexpr int jt = decltype(tc)::value;
      constexpr int q = PAR * 4 + jt;
      // loads younger than W(ft)[jt], oldest first: W(ft)[jt+1..3], W(ft+1)[0..3], W(ft+2)[0..jt-1] = 7
      asm volatile("s_waitcnt vmcnt(7)" : "+v"(ring[q])::"memory");
      static_for<8>([&](auto sc) __attribute__((always_inline)) {
        constexpr int s = decltype(sc)::value;
        acc[jt][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ring[q], af[PAR][s], acc[jt][s], 0, 0, 0);
      });
      __builtin_amdgcn_sched_barrier(0);
      SF_LOAD(ring[q], ft + 2, jt);
    });
  };
  auto chunk_mfma = [&](auto bufc, int cc) __attribute__((always_inline)) {
    constexpr int BUF = decltype(bufc)::value;  // = cc & 1; 9 cc has the same parity
    static_for<kSfTaps>([&](auto tapc) __attribute__((always_inline)) {
      constexpr int TAP = decltype(tapc)::value;
      tap_step(tapc, std::integral_constant<int, (BUF + TAP) & 1>{}, bufc, cc * kSfTaps + TAP);
    });
  };
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int s = 0; s < 8; ++s) acc[jt][s] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  // ---- epilogue of row tiles S0 .. S1 - 1: lane (c, g) holds positions p0 + 16 s + c, channels 64 wave + 16 jt + 4 g + r.  Stored
  // from that layout the tile leaves as 32-byte pieces (8 000 cycles per workgroup); staged through a wave-private LDS strip it leaves
  // as 128-byte row segments, 16 bytes per lane -----------------------------------------------------------------------------------------
  auto stage_store = [&](char* strip, const float4 (&bv)[4], int le, auto s0c, auto s1c) __attribute__((always_inline)) {
    constexpr int S0 = decltype(s0c)::value, S1 = decltype(s1c)::value;
#pragma unroll
    for (int s = S0; s < S1; ++s) {
      char* srow = strip + (16 * (s - S0) + c) * kSfOutPitch + 8 * gq;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const float v0 = fmaxf(acc[jt][s][0] + bv[jt].x, 0.f), v1 = fmaxf(acc[jt][s][1] + bv[jt].y, 0.f);
        const float v2 = fmaxf(acc[jt][s][2] + bv[jt].z, 0.f), v3 = fmaxf(acc[jt][s][3] + bv[jt].w, 0.f);
        *reinterpret_cast<uint2*>(srow + 32 * jt) = make_uint2(pack2_bf16(v0, v1), pack2_bf16(v2, v3));
      }
    }
    uint16_t* obase = p.out + ((int64_t)g.b * npos + g.p0) * kSfC + 64 * wave + 8 * (le & 7);
#pragma unroll
    for (int it = 2 * S0; it < 2 * S1; ++it) {
      const int m = 8 * it + (le >> 3);
      const uint4 v = *reinterpret_cast<const uint4*>(strip + (m - 16 * S0) * kSfOutPitch + 16 * (le & 7));
      if (m < g.np) *reinterpret_cast<uint4*>(obase + (int64_t)m * kSfC) = v;
    }
  };

  zero_acc();
  SF_LOAD(ring[0], 0, 0); SF_LOAD(ring[1], 0, 1); SF_LOAD(ring[2], 0, 2); SF_LOAD(ring[3], 0, 3);
  SF_LOAD(ring[4], 1, 0); SF_LOAD(ring[5], 1, 1); SF_LOAD(ring[6], 1, 2); SF_LOAD(ring[7], 1, 3);
  // Barriers here are RAW s_barrier: the W2 fragments in flight must stay in flight across them (a __syncthreads() would drain
  // vmcnt), and this wave's own LDS traffic is reads that its lgkmcnt(0) at a chunk's last tap has retired.  The producers' side
  // of the same barrier is a __syncthreads(), whose fence retires their patch writes.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's share of patch 0
  __builtin_amdgcn_s_barrier();  // B0: patch 0 is complete
  for (;;) {
    // A-fragment addresses: row tile s, lane (c, g) = output position p0 + 16 s + c, channels 8 g .. 8 g + 7 of the chunk
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      int m = 16 * s + c;
      if (m >= g.np) m = g.np - 1;
      const int pos = g.p0 + m, ho = pos / kSfF2, wo = pos - ho * kSfF2;
      a_addr[s] = (uint32_t)(uintptr_t)(lds_void_t*)(patch + ((2 * (ho - g.ho0)) * kSfF1 + 2 * wo) * kSfPitch + gq * 16);
    }
#pragma unroll 1
    for (int cc = 0; cc < kSfChunks; cc += 2) {
      SF_STAMP(4 + 2 * cc);
      chunk_mfma(std::integral_constant<int, 0>{}, cc);
      SF_STAMP(5 + 2 * cc);
      __builtin_amdgcn_s_barrier();  // patch cc + 1 is complete; every consumer is past its reads of patch cc
      SF_STAMP(6 + 2 * cc);
      chunk_mfma(std::integral_constant<int, 1>{}, cc + 1);
      SF_STAMP(7 + 2 * cc);
      if (cc + 2 < kSfChunks) __builtin_amdgcn_s_barrier();
    }
    const int tn = t + tstep;
    const bool more = WALK && tn < p.ntiles;
    if (!more)  // the loads past the last tap: their destination registers stay reserved until they have landed
      asm volatile("s_waitcnt vmcnt(0)"
                   : "+v"(ring[0]), "+v"(ring[1]), "+v"(ring[2]), "+v"(ring[3]), "+v"(ring[4]), "+v"(ring[5]), "+v"(ring[6]), "+v"(ring[7])
                   :
                   : "memory");
    // le = lane, b2p = p.b2, opaque per tile: the epilogue's address arithmetic and bias loads do not depend on the tile, and hoisted
    // out of the tile loop they would hold 50 registers through the main loop, which has none to spare
    int le = lane, zero = 0;
    asm volatile("" : "+v"(le), "+s"(zero));
    const float* b2p = p.b2 + zero;
    float4 bv[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) bv[jt] = *reinterpret_cast<const float4*>(b2p + 64 * wave + 16 * jt + 4 * (le >> 4));
    if constexpr (!WALK) {
      SF_STAMP(20);
      // The strips lie in the input rows / X / patch buffer 0, which nobody reads any more: the producers finished before the barrier
      // in front of the last chunk, and the last chunk's patch is buffer 1.
      stage_store(smem + wave * (kSfRows * kSfOutPitch), bv, le, std::integral_constant<int, 0>{}, std::integral_constant<int, 8>{});
      SF_STAMP(21);
      return;
    } else {
      __builtin_amdgcn_s_barrier();  // Bx: every consumer is past chunk 7 (its last tap ended on lgkmcnt(0)): buffer 1 is dead
      SF_STAMP(20);
      char* strip = patch + kSfPatchBytes + wave * ((kSfRows / 2) * kSfOutPitch);
      stage_store(strip, bv, le, std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{});
      stage_store(strip, bv, le, std::integral_constant<int, 4>{}, std::integral_constant<int, 8>{});
      SF_STAMP(21);
      if (!more) return;
      zero_acc();
      g = sf_tile(p, tn);
      t = tn;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of its strip
      __builtin_amdgcn_s_barrier();  // Bj: patch 0 of the next tile is complete; the producers may write buffer 1 again
      SF_NEXT_TILE();
      SF_STAMP(0);
    }
  }
#undef SF_LOAD
#undef SF_LDS
#undef SF_LDS8
}

#ifdef MA_SF_PROF
extern "C" int ma_debug_sf_prof(unsigned long long* host768) {
  return hipMemcpyFromSymbol(host768, HIP_SYMBOL(g_sf_prof), sizeof(unsigned long long) * 768) == hipSuccess ? 0 : -1;
}
#endif

MA_LDS_ATTR(subsample_fused_kernel<false>, kSfLds);
MA_LDS_ATTR(subsample_fused_kernel<true>, kSfLds);

}  // namespace ma

using namespace ma;

extern "C" int64_t ma_subsample_fused_packed_bytes(int64_t idim, int64_t C) {
  if (idim != kSfIdim || C != kSfC) return MA_ERR_UNSUPPORTED;
  return (int64_t)kSfW2Bytes + 16 * 1024;
}

extern "C" int ma_subsample_fused_pack_bf16(const float* W1, const void* W2, int64_t idim, int64_t C, void* packed, ma_stream_t stream) {
  if (!W1 || !W2 || !packed) return MA_ERR_INVALID_ARG;
  if (ma_subsample_fused_packed_bytes(idim, C) < 0) return MA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(W2) | reinterpret_cast<uintptr_t>(packed)) & 15) return MA_ERR_INVALID_ARG;
  const int total = 4 * kSfChunks * kSfTaps * 4 * 64 + 16 * 64;
  MA_LAUNCH(subsample_fused_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
            reinterpret_cast<const uint16_t*>(W2), W1, reinterpret_cast<uint4*>(packed));
  return MA_OK;
}

// The walking kernel is the default; MINDAUDIO_AMD_SUBSAMPLE=tile selects the one-tile-per-workgroup kernel for the whole process
// instead (same-library A/B, and the reference of tests/test_subsample_walk_gpu.py).  Read once.
static bool subsample_use_tile() {
  static const bool use = [] {
    const char* e = getenv("MINDAUDIO_AMD_SUBSAMPLE");
    return e && e[0] == 't' && e[1] == 'i' && e[2] == 'l' && e[3] == 'e';
  }();
  return use;
}

// max_workgroups < 0: the one-tile kernel; 0: as many workgroups as the device has compute units (one is resident per CU);
// n > 0: at most n workgroups (tests force long walks on small inputs with it).
static int subsample_fused_launch(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, int64_t batch, int64_t T,
                                  int32_t idim, const float* cmvn_mean, const float* cmvn_istd, const void* packed, const float* b1,
                                  const float* b2, int64_t C, void* out, int32_t max_workgroups, ma_stream_t stream) {
  if (!x || !packed || !b1 || !b2 || !out || batch < 1 || T < 7) return MA_ERR_INVALID_ARG;
  if ((cmvn_mean == nullptr) != (cmvn_istd == nullptr)) return MA_ERR_INVALID_ARG;
  if (ma_subsample_fused_packed_bytes(idim, C) < 0) return MA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(b2) |
       reinterpret_cast<uintptr_t>(b1)) & 15)
    return MA_ERR_INVALID_ARG;
  const int64_t T1 = (T - 3) / 2 + 1, Ho = (T1 - 3) / 2 + 1;
  const int64_t tiles = (Ho * kSfF2 + kSfRows - 1) / kSfRows;
  if (batch * tiles > 0x3fffffff || Ho > (1 << 24)) return MA_ERR_UNSUPPORTED;  // (tile index + grid size stays an int)
  SubsampleFusedParams p;
  p.x = x;
  p.sb = stride_b;
  p.st = stride_t;
  p.sf = stride_f;
  p.mean = cmvn_mean;
  p.istd = cmvn_istd;
  p.packed = reinterpret_cast<const char*>(packed);
  p.b1 = b1;
  p.b2 = b2;
  p.out = reinterpret_cast<uint16_t*>(out);
  p.Ho = (int32_t)Ho;
  p.tiles_per_utt = (int32_t)tiles;
  p.ntiles = (int32_t)(batch * tiles);
  if (max_workgroups < 0) {
    MA_LAUNCH(subsample_fused_kernel<false>, dim3((unsigned)p.ntiles), dim3(kSfThreads), kSfLds, (hipStream_t)stream, p);
  } else {
    const int wgs = max_workgroups > 0 ? max_workgroups : num_cus();
    MA_LAUNCH(subsample_fused_kernel<true>, dim3((unsigned)(p.ntiles < wgs ? p.ntiles : wgs)), dim3(kSfThreads), kSfLds,
              (hipStream_t)stream, p);
  }
  return MA_OK;
}

extern "C" int ma_subsample_fused_bf16(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, int64_t batch, int64_t T,
                                       int32_t idim, const float* cmvn_mean, const float* cmvn_istd, const void* packed, const float* b1,
                                       const float* b2, int64_t C, void* out, ma_stream_t stream) {
  return subsample_fused_launch(x, stride_b, stride_t, stride_f, batch, T, idim, cmvn_mean, cmvn_istd, packed, b1, b2, C, out,
                                subsample_use_tile() ? -1 : 0, stream);
}

extern "C" int ma_subsample_fused_walk_bf16(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, int64_t batch,
                                            int64_t T, int32_t idim, const float* cmvn_mean, const float* cmvn_istd, const void* packed,
                                            const float* b1, const float* b2, int64_t C, void* out, int32_t max_workgroups,
                                            ma_stream_t stream) {
  if (max_workgroups < 0) return MA_ERR_INVALID_ARG;
  return subsample_fused_launch(x, stride_b, stride_t, stride_f, batch, T, idim, cmvn_mean, cmvn_istd, packed, b1, b2, C, out,
                                max_workgroups, stream);
}
