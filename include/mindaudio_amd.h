/*
 * mindaudio_amd — C-ABI of the MI355X (gfx950) hot path of mindspore-lab/mindaudio.
 *
 * mindaudio has no FFI/plugin layer of its own (it is 100 % Python); the
 * boundary it offers is its Python call signatures.  Each entry point below replaces the
 * native arithmetic behind one of those signatures and is what a binding in the reference
 * (ctypes) would call.  Conventions:
 *
 *   - plain C, no torch / C++ types; every pointer marked "device" is HBM memory of the
 *     current HIP device, everything else is a host scalar;
 *   - no allocation, no synchronisation inside: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = default stream) and the call returns;
 *   - return value: MA_OK or a negative MA_ERR_* code; the Python mirror maps the codes to
 *     the exceptions the reference raises (ValueError for n_fft > len, hop < 1, ...).
 *
 * All shapes are row-major unless stated.
 */
#ifndef MINDAUDIO_AMD_H_
#define MINDAUDIO_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an existing entry point changes its argument list, its meaning or the size a caller has to provide, or is removed
 * (new entry points alone do not bump it).
 * 2: ma_fbank_kaldi_f32 gained `frames_out`; ma_ffn_bf16 / ma_ffn128_bf16 / ma_ffn_ln_bf16 / ma_layernorm*_add_f32 were removed
 *    (round 2).
 * 3: ma_ctc_grad_workspace_bytes returns twice the size (alpha and beta side by side, round 4); ma_ffn_train_bf16 accepts ldu == 0
 *    (no tape: u / h are scratch rows); ma_init is per device ordinal; ma_subsample_fused_pack_bf16 takes the float32 conv1 weight
 *    (round 5); ma_attn_out_convmodule_bf16 writes x_out instead of updating x in place (round 5).
 * 4: the development hook of the two-queue corruption hunt (a dynamic-LDS override of the grouped split-K launch) was removed.
 * The Python binding refuses a library of another version (mindaudio_amd/_lib.py). */
#define MA_ABI_VERSION 4

typedef void* ma_stream_t; /* hipStream_t */

enum ma_status {
  MA_OK = 0,
  MA_ERR_INVALID_ARG = -1,   /* null pointer, non-positive size, unsupported enum */
  MA_ERR_NFFT_TOO_LARGE = -2, /* n_fft > signal length: spectrum.py:182-187, :243-246 */
  MA_ERR_HOP = -3,            /* hop < 1: spectrum.py:295-296 */
  MA_ERR_WINDOW = -4,         /* win_length > n_fft: spectrum.py:331-334 */
  MA_ERR_UNSUPPORTED = -5,    /* valid request that this build has no kernel for */
  MA_ERR_LAUNCH = -6,         /* hipLaunch / hipGetLastError failure */
  MA_ERR_WORKSPACE = -7       /* workspace too small */
};

/* np.pad modes the reference forwards (stft: pad_mode, spectrum.py:132; Spectrogram:
 * BorderType, spectrum.py:671). */
enum ma_pad_mode { MA_PAD_CONSTANT = 0, MA_PAD_REFLECT = 1, MA_PAD_EDGE = 2, MA_PAD_SYMMETRIC = 3 };

/* Output layout of ma_stft_f32. */
enum ma_stft_layout {
  MA_STFT_FRAME_MAJOR = 0, /* (batch, n_frames, n_freq) complex64 — for a 1-D wave this is exactly the
                              Fortran-ordered (n_freq, n_frames) array of spectrum.py:252 */
  MA_STFT_FREQ_MAJOR = 1   /* (batch, n_freq, n_frames) complex64, C order */
};

int ma_abi_version(void);
const char* ma_status_string(int status);

/* Set-up of the library's kernels on the CURRENT device (the raised dynamic-LDS limit of every kernel that needs one, all in one go;
 * the runtime keeps the attribute per device, so it is applied once per device ordinal).  Needs a HIP device; idempotent and thread-safe.  Every launch entry point calls it implicitly, so calling it is optional -
 * a host that wants no runtime configuration call after start-up (e.g. before it starts a second stream) calls it once.
 * (The reference has no counterpart: it is pure Python, mindaudio/__init__.py.)  ma_init_kernel_attributes() = how many
 * kernels are registered (a load-time constant; the CPU test checks that the registrations were linked in). */
int ma_init(void);
int32_t ma_init_kernel_attributes(void);

/* Measurement aid of bench.py (roofline_fbank.valu), not part of the drop-in path: `iters` x 16 independent v_fma_f32 per wave on
 * `wgs_per_cu` resident 4-wave workgroups per CU.  Timed by the caller: ns per wave-instruction per SIMD = t / (16 iters wgs_per_cu). */
int ma_valu_issue_probe(int32_t wgs_per_cu, int32_t iters, float* sink, ma_stream_t stream);
/* Measurement aid of bench.py (roofline.weight_stream): one 4-wave workgroup per CU, every wave streams `rounds` x 16 fragments of
 * 1 KiB from `buf` (bytes % 4096 == 0; wave w walks quarter w, all CUs the same bytes: L2-resident like a packed weight) through a
 * 16-slot register ring with 4 MFMAs per fragment - the main-loop pattern of ffn_packed_kernel.  GB/s per CU = 65536 rounds / t. */
int ma_weight_stream_probe(const void* buf, int64_t bytes, int32_t rounds, float* sink, ma_stream_t stream);

/* 1 + n // hop (center) or 1 + (n - n_fft) // hop — spectrum.py:196,298; <0 on invalid args. */
int64_t ma_num_frames(int64_t n, int32_t n_fft, int32_t hop, int32_t center);

/*
 * Triangular mel filterbank in grouped band form.  Built on the host in float64 (HTK bank of MelScale,
 * spectrum.py:686-694; Kaldi bank of dataset.py:68-113), rounded to float32 and uploaded once.
 *
 * Filters are taken eight at a time: "row" i holds filters 8i .. 8i+7 (g = m % 8 is the lane group that
 * evaluates filter m).  Every filter of a row is evaluated over the same number steps[i] of 4-bin steps
 * (the widest filter of the row decides; the others carry zero weights), so the mel loop has wave-uniform
 * trip counts and reads bins and weights 16 bytes at a time:
 *
 *   mel[m = 8i+g] = sum_{s < steps[i]} sum_{c < 4} weights[((row_off[i] + s) * 8 + g) * 4 + c]
 *                                                 * spectrum[start[8i+g] + 4s + c]
 *
 * Contract: start[] % 4 == 0 and start[8i+g] + 4*steps[i] <= ma_mel_row_stride(n_fft) (260 for n_fft = 512; the
 * kernels keep the bins from n_freqs up to that stride at zero); row_off is the exclusive prefix sum of steps;
 * filters >= n_mels in the last row have zero weights.
 */
typedef struct ma_melbank {
  int32_t n_mels;
  int32_t n_freqs;          /* n_fft / 2 + 1 */
  int32_t n_rows;           /* ceil(n_mels / 8) */
  int32_t total_steps;      /* sum of steps[] */
  const int32_t* steps;     /* device, [n_rows] */
  const int32_t* row_off;   /* device, [n_rows] */
  const int32_t* start;     /* device, [n_rows * 8] */
  const float* weights;     /* device, [total_steps * 8 * 4] */
} ma_melbank_t;

/* Row length (floats) of the kernels' spectrum tile for this n_fft: the `row_limit` of the grouped bank above.
 * n_fft = 512 is the FFT fast path; any other even n_fft in [4, 1024] (the reference's default n_fft = 400,
 * features.py:201, spectrum.py:611) runs the exact-f32 MFMA DFT path.  <0 when unsupported. */
int32_t ma_mel_row_stride(int32_t n_fft);

/*
 * spectrum.stft (mindaudio/data/spectrum.py:125-278), batched.
 *   wav     device (batch, n) float32, row stride `wav_stride` elements
 *   window  device (n_fft,) float32: scipy get_window(..., fftbins=True) centred-padded to
 *           n_fft by the host (spectrum.py:173-175)
 *   out     device complex64 as interleaved float pairs, layout per `layout`
 * n_frames = ma_num_frames(n, n_fft, hop, center).
 */
int ma_stft_f32(const float* wav, int64_t batch, int64_t n, int64_t wav_stride,
                int32_t n_fft, int32_t hop, const float* window,
                int32_t center, int32_t pad_mode, int32_t layout,
                float* out, ma_stream_t stream);

/* Bytes of device workspace ma_fbank_db_f32 / ma_fbank_kaldi_f32 need. */
int64_t ma_fbank_workspace_bytes(int64_t batch, int64_t n_frames);

/*
 * features.fbank with deltas=False, context=False (mindaudio/data/features.py:196-270):
 * melspectrogram (spectrum.py:609-698: centred power spectrogram -> mel bank) followed by
 * amplitude_to_dB (spectrum.py:25-90), fused.
 *   out[b, m, t] = mult*log10(max(mel, amin)) - db_offset, then, if top_db >= 0,
 *   max(out, max_over_the_whole_call(out) - top_db)   (batch-global floor, spectrum.py:79-89)
 *   power: exponent of |X| (1.0 or 2.0);  db_offset = mult*log10(max(amin, |ref|)).
 *   out     device (batch, n_mels, n_frames) float32
 *   workspace device, >= ma_fbank_workspace_bytes(batch, n_frames)
 */
int ma_fbank_db_f32(const float* wav, int64_t batch, int64_t n, int64_t wav_stride,
                    int32_t n_fft, int32_t hop, const float* window,
                    int32_t center, int32_t pad_mode, const ma_melbank_t* mel,
                    float power, float mult, float amin, float db_offset, float top_db,
                    float* out, void* workspace, int64_t workspace_bytes, ma_stream_t stream);

/* Same front end, no dB: spectrum.melspectrogram (spectrum.py:609-698). out (batch, n_mels, n_frames). */
int ma_melspectrogram_f32(const float* wav, int64_t batch, int64_t n, int64_t wav_stride,
                          int32_t n_fft, int32_t hop, const float* window,
                          int32_t center, int32_t pad_mode, const ma_melbank_t* mel, float power,
                          float* out, ma_stream_t stream);

/*
 * Kaldi-style log-mel of the Conformer data loader, batched on device
 * (examples/conformer/dataset.py:117-168 compute_fbank_feats; replaces the Pool(8) of :449,479).
 *   wav      device (batch, max_n) float32, already scaled by 2^15 (dataset.py:390)
 *   lengths  device (batch,) int64 valid samples per utterance
 *   window   device (frame_len,) float32 = hanning(frame_len)^0.85 (dataset.py:126)
 *   out      device (batch, max_frames, n_mels) float32, rows t >= frames(b) are zero
 *            (pad_sequence padding value, dataset.py:563-569); max_frames = (max_n - frame_len)/shift + 1
 *   frames_out  device (batch,) int64, frames of each utterance (what the loader keeps as xs_lengths), or NULL
 * Per utterance: pre-emphasis over the whole signal, framing without centring, window,
 * subtraction of ONE scalar mean over all windowed frames (dataset.py:165), zero-pad to n_fft,
 * |rFFT|^2, mel bank, zeros -> eps, natural log.
 */
int ma_fbank_kaldi_f32(const float* wav, const int64_t* lengths, int64_t batch, int64_t max_n,
                       int64_t wav_stride, int32_t frame_len, int32_t frame_shift, int32_t n_fft,
                       const float* window, const ma_melbank_t* mel, float preemph,
                       float* out, int64_t* frames_out, void* workspace, int64_t workspace_bytes,
                       ma_stream_t stream);

/* Bytes of device workspace ma_amplitude_to_db_f32 needs. */
int64_t ma_db_workspace_bytes(int64_t groups, int64_t elems_per_group);

/* spectrum.amplitude_to_dB on a device array viewed as (groups, elems_per_group): the top_db floor is
 * taken per group (spectrum.py:79-89: one group per leading index after the reshape). In place allowed. */
int ma_amplitude_to_db_f32(const float* in, int64_t groups, int64_t elems_per_group,
                           float mult, float amin, float db_offset, float top_db,
                           float* out, void* workspace, int64_t workspace_bytes, ma_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Conformer encoder building blocks (mindaudio/models/conformer.py, mindaudio/models/layers/...).
 * Activations that feed a matmul are bf16 (stored as uint16 bit patterns), the residual stream and all
 * reductions are float32; every matmul accumulates in float32 on the MFMA units.
 * ---------------------------------------------------------------------------------------------- */

/* What happens to acc = A . W^T before it is stored:
 *   v = act2(act(acc + bias[n]) * col_scale[n] + col_shift[n]) * alpha * row_scale[m] (+ residual[m, n])
 * act / act2: 0 none, 1 swish x*sigmoid(x) (layers/swish.py:14-16), 2 relu, 3 sigmoid, 4 tanh.  NULL pointers switch a
 * term off.  col_scale/col_shift: a BatchNorm in affine form behind the activation (ecapatdnn.py:60-64: conv -> ReLU ->
 * BatchNorm). */
typedef struct ma_gemm_epilogue {
  const float* bias;       /* device [N] */
  const float* residual;   /* device (M, N) float32, row stride ldr */
  const float* row_scale;  /* device [M]: the mask_pad multiply of layers/convolution.py:97-98,126-127 */
  int64_t ldr;
  float alpha;             /* e.g. ff_scale 0.5 (models/conformer.py:69) or sqrt(d_model) (embedding.py:84) */
  int32_t act;
  int32_t out_bf16;        /* 1: out is bf16, 0: float32 */
  const float* col_scale;  /* device [N], 16-byte aligned; NULL: no affine */
  const float* col_shift;  /* device [N] */
  int32_t act2;
  int32_t reserved;
} ma_gemm_epilogue_t;

/* Dense / k=1 Conv1d (layers/dense.py:51-58, layers/conv1d.py): out (M, N) = epilogue(A (M, K) . W (N, K)^T).
 * A, W device bf16 with K contiguous (W is the (out, in) weight as stored by the reference), K % 64 == 0,
 * lda/ldw multiples of 8, 16-byte aligned bases. */
int ma_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* out, int64_t ldo,
                 int64_t M, int64_t N, int64_t K, const ma_gemm_epilogue_t* epi, ma_stream_t stream);

/* Which kernel ma_gemm_bf16 would run for these arguments: a host-side query that launches nothing (tests assert through it that a
 * shape reaches the kernel they mean to test).  `out` is read for its alignment only; `cus` is the compute-unit count to decide for
 * (<= 0: the current device's).  Returns a negative MA_ERR_* where ma_gemm_bf16 would refuse the same arguments, else
 *   MA_GEMM_KERNEL_* | MA_GEMM_VARIANT_EPI1 (the instantiation with the column affine / second activation / sigmoid / tanh)
 *                    | im2col << MA_GEMM_VARIANT_IM2COL_SHIFT (0 plain A, 1 the 3x3 stride-2 Conv2d, 2 Conv1d taps)
 *                    | MA_GEMM_VARIANT_NT (bf16 tiles leave through non-temporal stores).
 * The launch switches on the same decision: the two cannot disagree. */
#define MA_GEMM_KERNEL_WS512 1          /* weight-stationary, K = 512 */
#define MA_GEMM_KERNEL_8PH_ROWMAJOR 2   /* 256 x 256 tiles, 8-phase schedule, row-major tile order */
#define MA_GEMM_KERNEL_8PH_BLOCKED 3    /* ... blocked tile order */
#define MA_GEMM_KERNEL_TILE_128X128X2 4 /* 128 x 128 tiles, 2-stage ring */
#define MA_GEMM_KERNEL_TILE_64X128X2 5  /* 64 x 128 tiles, 2-stage ring */
#define MA_GEMM_KERNEL_TILE_64X128X3 6  /* 64 x 128 tiles, 3-stage ring */
#define MA_GEMM_KERNEL_TILE_128X128X3 7 /* development builds only */
#define MA_GEMM_VARIANT_KERNEL_MASK 0xf
#define MA_GEMM_VARIANT_EPI1 0x10
#define MA_GEMM_VARIANT_IM2COL_SHIFT 5
#define MA_GEMM_VARIANT_NT 0x100
int32_t ma_gemm_bf16_variant(int64_t M, int64_t N, int64_t K, int64_t ldo, const ma_gemm_epilogue_t* epi, const void* out,
                             int32_t cus);

/* 3x3, stride 2, valid Conv2d (layers/subsampling.py:43) as an implicit GEMM.
 *   act device bf16 NHWC (batch, H, Wd, C), C % 64 == 0;  W device bf16 (Cout, 3, 3, C) i.e. k = (kh, kw, c);
 *   out (batch, Ho, Wo, Cout), Ho = (H-3)/2+1, Wo = (Wd-3)/2+1, dtype per epilogue. */
int ma_conv2d_3x3s2_nhwc_bf16(const void* act, int64_t batch, int64_t H, int64_t Wd, int64_t C, const void* W,
                              int64_t Cout, void* out, const ma_gemm_epilogue_t* epi, ma_stream_t stream);

/* LayerNorm of layers/layernorm.py:53-60: (x - mean) / sqrt(biased_var + eps) * gamma + beta, one row per
 * wave; optional row_scale[m] multiply (the `x * mask` in front of pointwise_conv1, convolution.py:97-98).
 * x (rows, cols) float32; out bf16 or float32; cols in {256, 512, 768, 1024}. */
int ma_layernorm_f32(const float* x, int64_t ldx, int64_t rows, int64_t cols, const float* gamma,
                     const float* beta, float eps, const float* row_scale, void* out, int64_t ldo,
                     int32_t out_bf16, ma_stream_t stream);

/* Two chained LayerNorms in one pass over 256-wide rows: out1 = LN(x; gamma1, beta1) float32 (may alias x),
 * out2 = LN(out1; gamma2, beta2) bf16 or float32 — norm_final of one block followed by norm_ff_macaron of the
 * next, or by after_norm (models/conformer.py:155-156, 109-110, 253-254). */
int ma_layernorm2_f32(const float* x, int64_t ldx, int64_t rows, int64_t cols, const float* gamma1,
                      const float* beta1, const float* gamma2, const float* beta2, float eps, float* out1,
                      int64_t ldo1, void* out2, int64_t ldo2, int32_t out2_bf16, ma_stream_t stream);

/* GlobalCMVN (layers/cmvn.py:33-35; mean/istd may be NULL) + Conv2d(1 -> C, 3x3, stride 2, valid) + ReLU
 * (layers/subsampling.py:41-42).  x (batch, T, idim) float32; w (C, 3, 3), bias (C) float32;
 * out NHWC bf16 (batch, (T-3)/2+1, (idim-3)/2+1, C). */
int ma_subsample_conv1_nhwc(const float* x, int64_t batch, int64_t T, int32_t idim, const float* cmvn_mean,
                            const float* cmvn_istd, const float* w, const float* bias, int32_t C, void* out,
                            ma_stream_t stream);
/* The same on a strided view x[b * stride_b + t * stride_t + f * stride_f] (element strides): lets the encoder take
 * features.fbank's (batch, n_mels, frames) output as (batch, frames, n_mels) without a transposing copy. */
int ma_subsample_conv1_strided_nhwc(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, int64_t batch, int64_t T,
                                    int32_t idim, const float* cmvn_mean, const float* cmvn_istd, const float* w,
                                    const float* bias, int32_t C, void* out, ma_stream_t stream);

/* RelPositionMultiHeadedAttention core (layers/attention.py:214-235 + 100-113), one fused kernel:
 *   score = ((q + u) k^T + (q + v) p^T) / sqrt(d_k) + (mask == 0) * -10000 ; softmax ; . v     (no rel-shift)
 *   qkv  device bf16 (batch*T, >= 768): columns [0,256) q, [256,512) k, [512,768) v, head h at h*64
 *   pos  device bf16 (T, 256): linear_pos(pos_emb), shared by the batch (attention.py:210-211,230)
 *   bias_u / bias_v float32 (heads, 64); mask float32 (batch, T) or NULL; ctx bf16 (batch*T, 256);
 *   vt_workspace: device scratch of ma_relpos_attention_workspace_bytes() (reserved: V is now read from qkv as stored, with
 *   transposing LDS reads; the buffer is not written). */
int64_t ma_relpos_attention_workspace_bytes(int64_t batch, int64_t T, int32_t heads, int32_t d_k);
int ma_relpos_attention_bf16(const void* qkv, int64_t ld_qkv, const void* pos, int64_t ld_pos,
                             const float* bias_u, const float* bias_v, const float* mask, int64_t batch,
                             int64_t T, int32_t heads, int32_t d_k, void* ctx, int64_t ld_ctx,
                             void* vt_workspace, int64_t vt_workspace_bytes, ma_stream_t stream);
/* The same with a per-(query, key) mask (batch, T, T) float32 (0 = masked, the additive -10000 of the padding mask): the
 * chunk masks of the streaming encoder configuration (mindaudio/utils/mask.py:201-271 add_optional_chunk_mask, applied at
 * layers/attention.py:102-108); the padding mask is expected to be folded in, as the reference does (masks & chunk_masks). */
int ma_relpos_attention_qmask_bf16(const void* qkv, int64_t ld_qkv, const void* pos, int64_t ld_pos,
                             const float* bias_u, const float* bias_v, const float* mask_qk, int64_t batch,
                             int64_t T, int32_t heads, int32_t d_k, void* ctx, int64_t ld_ctx,
                             void* vt_workspace, int64_t vt_workspace_bytes, ma_stream_t stream);

/* Middle of ConvolutionModule (layers/convolution.py:100-121): GLU(dim=channels) -> depthwise Conv1d(k, same
 * zero padding per utterance) -> BatchNorm1d in affine form -> Swish.
 *   y (batch*T, 2C) bf16 = pointwise_conv1 output; dw (C, k) float32; out (batch*T, C) bf16
 *   bn_scale = gamma / sqrt(var + eps), bn_shift = beta + (dw_bias - mean) * bn_scale  (host-folded). */
int ma_convmodule_mid_bf16(const void* y, int64_t ldy, int64_t batch, int64_t T, int32_t C, const float* dw,
                           int32_t kernel_size, const float* bn_scale, const float* bn_shift, void* out,
                           int64_t ldo, ma_stream_t stream);

/* CTC branch, forward value (mindaudio/loss/ctc_loss.py:53-64): float32 log_softmax over V + CTCLossV2(blank,
 * reduction none, zero_infinity) + sum over the batch / batch.
 *   logits (batch*T, V) float32 row stride ld (= ctc_lo output, ma_gemm_bf16 with float32 out);
 *   ys (batch, Lmax) int32 padded labels; hlens / ylens (batch) int32 input / target lengths;
 *   per_utt_loss (batch) float32 out; lse_workspace (batch*T) float32; loss_out (1) float32.
 * Targets up to 223 labels (2*Lmax + 1 <= 448; up to 127 on the 4-chunk form, longer ones - the data set classes default to
 * token_max_length 200, the shipped conformer.yaml sets 30 - on a 7-chunk instantiation of the same recursion, round 6). */
int ma_ctc_loss_f32(const float* logits, int64_t ld, int64_t batch, int64_t T, int32_t V, const int32_t* ys,
                    int32_t Lmax, const int32_t* hlens, const int32_t* ylens, int32_t blank,
                    int32_t zero_infinity, float* per_utt_loss, float* lse_workspace, float* loss_out,
                    ma_stream_t stream);

/* Loss value AND gradient of the CTC branch: as ma_ctc_loss_f32, plus dlogits (batch*T, ld_out) bf16 =
 * grad_scale * d(sum of per-utterance CTC) / d logits (softmax - state occupancies; zero for frames past hlens and
 * for utterances whose loss is infinite — zero_infinity must be on).  Columns [V, ld_out) are zero-filled so the buffer
 * can be a K-padded GEMM operand.  workspace >= ma_ctc_grad_workspace_bytes (the log alpha and log beta lattices: the two recursions run
 * side by side in one launch, round 4). */
int64_t ma_ctc_grad_workspace_bytes(int64_t batch, int64_t T, int32_t Lmax);
int ma_ctc_loss_grad_f32(const float* logits, int64_t ld, int64_t batch, int64_t T, int32_t V, const int32_t* ys,
                         int32_t Lmax, const int32_t* hlens, const int32_t* ylens, int32_t blank,
                         int32_t zero_infinity, float grad_scale, float* per_utt_loss, float* lse_workspace,
                         float* loss_out, void* dlogits, int64_t ld_out, void* workspace, int64_t workspace_bytes,
                         ma_stream_t stream);

/* CTC greedy search (models/decoders/decoder_factory.py:9-56 + utils/recognize.py:254-270): per frame the arg-max class
 * of log_softmax(logits) (first index on ties) and its log-probability; frames with mask == 0 (mask (batch*T) float32,
 * optional) become 0 = blank as in `topk_index * encoder_mask`; then remove_duplicates_and_blank
 * (utils/common.py:116-125) per utterance: hyp (batch, T) int32 zero padded, hyp_len (batch). */
int ma_ctc_greedy_search_f32(const float* logits, int64_t ld, int64_t batch, int64_t T, int32_t V, const float* mask,
                             int32_t blank, int32_t* best, float* best_logp, int32_t* hyp, int32_t* hyp_len,
                             ma_stream_t stream);

/* CTC top-k (the ops.TopK(ctc_probs, beam_size) of CTCPrefixBeamSearch, models/decoders/decoder_factory.py:195-239): per row of
 * logits (rows, V) float32 with row stride ld, the k largest values of log_softmax(row) in descending order, equal values lower
 * index first: topk_logp / topk_index (rows, k) contiguous.  One wave per row.  1 <= k <= 16 and k <= V, else MA_ERR_UNSUPPORTED
 * (k > 16) / MA_ERR_INVALID_ARG. */
int ma_ctc_topk_f32(const float* logits, int64_t ld, int64_t rows, int32_t V, int32_t k, float* topk_logp, int32_t* topk_index,
                    ma_stream_t stream);

/* CTC prefix beam search (utils/recognize.py:273-336), batched: one workgroup per utterance, one launch for the batch.
 *   topk_logp (batch, T, beam) float32 / topk_index (batch, T, beam) int32: ma_ctc_topk_f32 with k = beam (indices of a frame
 *     distinct, as TopK gives them); mask (batch*T) float32 or NULL: frames with mask == 0 are skipped wherever they are.
 *   Per frame, for every (top-k entry s, hypothesis) pair in the reference's loop order: s == blank -> pb of the prefix; s == the
 *   prefix's last token -> pnb of the prefix from pnb and pnb of prefix + s from pb; otherwise pnb of prefix + s from pb and pnb.
 *   float64 arithmetic with the reference's log_add (argument order kept); the candidates ranked by log_add(pb, pnb) descending,
 *   ties in first-touch order, the first `beam` kept.  Prefixes are compared exactly (a 64-bit hash only filters).
 *   hyp (batch, beam, T) int32 (a hypothesis slot's tokens, zero padded), hyp_len (batch, beam), score (batch, beam) float64 =
 *   log_add(pb, pnb), n_hyp (batch): how many hypotheses survived (<= beam: an utterance with one valid frame may have fewer;
 *   slots past n_hyp hold length 0 and score -inf).
 * Limits: 1 <= beam <= 16 and 2 * beam * T * 4 bytes of prefix tokens (double buffered in LDS) <= 144 KiB (beam 16: T <= 1152),
 * else MA_ERR_UNSUPPORTED. */
int ma_ctc_prefix_beam_search_f32(const float* topk_logp, const int32_t* topk_index, const float* mask, int64_t batch, int32_t T,
                                  int32_t beam, int32_t blank, int32_t* hyp, int32_t* hyp_len, double* score, int32_t* n_hyp,
                                  ma_stream_t stream);

/* The score loop of attention_rescoring (utils/recognize.py:393-406) for n_utt utterances of `group` hypotheses each:
 *   logits (n_utt*group*L1, V) float32 with row stride ld (the decoder's scores before log_softmax), tokens (n_utt*group, ld_tok)
 *   int32 with lens (n_utt*group) <= L1 - 1, ctc_score (n_utt*group) float64, n_hyp (n_utt) int32 or NULL (all valid): hypotheses
 *   h >= n_hyp[b] of an utterance are skipped.
 *   hyp_score[h] = sum_{j < len} logp[j][tok_j] + logp[len][eos] + ctc_weight * ctc_score[h] summed in float64 in that order, logp
 *   the row's log_softmax (one wave per row; -inf for a skipped hypothesis, NaN for a length or token out of range);
 *   best_index / best_score (n_utt): the first hypothesis with the highest score (a later one wins only if strictly greater; 0 and
 *   -inf when none is valid).  workspace >= n_utt*group*L1 float64.  Two launches. */
int ma_hyp_score_f32(const float* logits, int64_t ld, int32_t V, int64_t n_utt, int32_t group, int32_t L1, const int32_t* tokens,
                     int64_t ld_tok, const int32_t* lens, const int32_t* n_hyp, int32_t eos, const double* ctc_score,
                     double ctc_weight, double* workspace, double* hyp_score, int32_t* best_index, double* best_score,
                     ma_stream_t stream);

/* ---- the autoregressive `attention` decode mode (utils/recognize.py:78-251, decoder_factory.py:59-192, 278-413) --------------
 * One decode step of the decoder's self-attention on a key / value cache, with the beam reorder and the append in the launch:
 *   qkv (R, 3 d) bf16 with row stride ldqkv: row r's new query | key | value, R = batch * beam, d = heads * 64;
 *   k_in, v_in (R, Lmax, d) bf16 contiguous: the cache as the previous step left it, t cached positions, 0 <= t < Lmax;
 *   parent (R) int32 or NULL (the identity): the cache row that row r continues (values outside [0, R) are clamped into it).
 *   k_out[r, 0:t] = k_in[parent[r], 0:t] bit for bit, k_out[r, t] = the new key; v_out likewise; positions above t of the out
 *   cache are not written.  ctx (R, d) bf16 with row stride ldc: softmax(scale * q . k_j, j <= t) v with no mask (every cached key
 *   is valid).  In and out are different buffers (the caller alternates two by the step's parity): two children may share a parent,
 *   the launch never reads what it writes, the stream order is the only synchronisation, and there are no atomics - two runs
 *   give the same bits.
 * Rounding points, those of ma_mha_small_fwd_bf16: q, k, v are bf16 and their products exact in float32; scores (float32 fma
 * sums, then * scale), the row maximum, exp and the sum are float32 (__expf: a key more than 104 below the row maximum weighs
 * exactly 0); the normalised probability is rounded to bf16 (the operand of the P V product); the P V sum is float32; ctx is
 * rounded to bf16 once.  One wave per (row, head); the launch is bound by latency, not by bandwidth or the matrix pipe.
 * MA_ERR_UNSUPPORTED: d_k != 64, d != heads * 64, Lmax > 2048, a row stride that is no multiple of 8.  MA_ERR_INVALID_ARG:
 * t >= Lmax, R == 0, a NULL or not 16-byte aligned buffer, an in buffer that overlaps an out buffer. */
int ma_decoder_self_attn_step_bf16(const void* qkv, int64_t ldqkv, const void* k_in, const void* v_in, const int32_t* parent,
                                   int64_t R, int32_t Lmax, int32_t t, int32_t heads, int32_t d_k, int32_t d, float scale, void* ctx,
                                   int64_t ldc, void* k_out, void* v_out, ma_stream_t stream);

/* Steps 2.2-2.6 of the attention beam search (PredictNet.construct, decoder_factory.py:387-413, and recognize.py:236-242) for a
 * batch: one workgroup per utterance, one launch, no atomics.  N = beam, rows u * N .. u * N + N - 1 belong to utterance u.
 *   topk_logp / topk_index (batch * N, N): ma_ctc_topk_f32 of the step's logits with k = N (1 <= N <= 16, N <= V);
 *   scores_in (batch * N) float32, end_in (batch * N) int32, tokens_in (batch * N, W) int32 with sos in column 0,
 *   length (batch) int32: tokens generated so far, done (batch) int32; max_new <= W - 1 (the reference's maxlen - 1).
 * Per utterance that is not done, in float32: candidate (r, j) = scores[r] + m, m = logp[r][j] for an unfinished row; for a
 * finished row m is exactly +0.0 for j == 0 and logp[r][j] + (-10000.0f) for j > 0, and its token is eos (mask_finished_scores /
 * mask_finished_preds; -10000 is the reference's constant.  The reference multiplies the finished row's first logp by 0, which is
 * NaN for an infinite logp; here that branch ADDS 0).  The N best of the N * N candidates in descending order, equal values lower
 * flat index r * N + j first (the reference's topk_fun is a stable sort), -inf last (NaN ranks as -inf).  For output slot s:
 * scores_out[s] = the candidate's value, parent[s] = its GLOBAL row index, pred[s] = its token, tokens_out[s] = tokens_in[parent[s]]
 * with column length + 1 set to the token, end_out[s] = (token == eos).  Then length += 1 and done = 1 when every end_out of the
 * utterance is set or length >= max_new.
 * An utterance that is done is frozen: scores, flags and tokens are copied through, parent is the identity, pred is eos, length
 * stays - so every utterance of a batch gets the result of a one-utterance call.  (The reference goes on appending eos to a finished
 * utterance until the whole batch has finished; that is deliberately not kept.)  The in and out arrays must not overlap; length
 * and done are updated in place; the host reads `done`.  beam > 16: MA_ERR_UNSUPPORTED. */
int ma_attn_beam_step_f32(const float* topk_logp, const int32_t* topk_index, const float* scores_in, const int32_t* end_in,
                          const int32_t* tokens_in, int64_t batch, int32_t beam, int32_t W, int32_t eos, int32_t max_new,
                          int32_t* length, int32_t* done, float* scores_out, int32_t* end_out, int32_t* tokens_out, int32_t* parent,
                          int32_t* pred, ma_stream_t stream);

/* topk_fun(scores, 1) of the search's end (recognize.py:244-251): per utterance the first slot with the highest score;
 * best_hyp (batch, W - 1) int32 = that slot's token row without column 0, best_len (batch) = length, best_score (batch) float32. */
int ma_attn_beam_best_f32(const float* scores, const int32_t* tokens, const int32_t* length, int64_t batch, int32_t beam, int32_t W,
                          int32_t* best_hyp, int32_t* best_len, float* best_score, ma_stream_t stream);

/* float32 -> bf16 (round to nearest even), n % 4 == 0: the `cast` in front of a matmul operand. */
int ma_cast_f32_bf16(const float* x, void* y, int64_t n, ma_stream_t stream);

/* nn.Conv1d(C -> N, kernel `taps`, dilation, pad_mode "same") of mindaudio/models/ecapatdnn.py:47-56 as an implicit
 * GEMM over a (rows, C) bf16 activation with row stride lda:
 *   out[m, n] = epilogue( sum_{j < taps} sum_{c < C} act[m + (j - taps/2) * dilation, c] * W[n, j, c] )
 * W (N, taps, C) bf16.  "Same" zero padding comes from the layout: every utterance is stored with >= (taps/2)*dilation
 * zero halo rows before and after it (and the buffer with that many margin rows at both ends), and the epilogue's
 * row_scale zeroes the halo rows of the output so that it can feed the next convolution.  C % 64 == 0. */
int ma_conv1d_taps_bf16(const void* act, int64_t lda, int64_t rows, int64_t C, int32_t taps, int32_t dilation,
                        const void* W, void* out, int64_t ldo, int64_t N, const ma_gemm_epilogue_t* epi,
                        ma_stream_t stream);

/* The kernel ma_conv1d_taps_bf16 would run: the sibling of ma_gemm_bf16_variant, same encoding (taps == 1 is a plain GEMM). */
int32_t ma_conv1d_taps_bf16_variant(int64_t rows, int64_t C, int32_t taps, int32_t dilation, int64_t ldo, int64_t N,
                                    const ma_gemm_epilogue_t* epi, const void* out, int32_t cus);

/* ---- ECAPA-TDNN forward (mindaudio/models/ecapatdnn.py:7-433): the pieces between its convolutions ------------
 * Activations: (batch, T + 2*halo, C) bf16, zero halo frames around every utterance (see ma_conv1d_taps_bf16). */

/* (batch, T, F) float32 features -> (batch, T + 2*halo, Cpad) bf16, zero halo frames and zero channels F..Cpad-1. */
int ma_ecapa_pack_input_bf16(const float* x, int64_t batch, int64_t T, int32_t F, int32_t halo, int32_t Cpad, void* out,
                             ma_stream_t stream);
/* out = a + b on (rows, cols) bf16 slices with their own row strides (Res2Net's x_i + y_{i-1}, ecapatdnn.py:108-111);
 * b == NULL: strided copy.  cols and strides multiples of 8. */
int ma_add_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo, int64_t rows, int64_t cols,
                ma_stream_t stream);
/* SE squeeze (ecapatdnn.py:152-153): out (batch, C) bf16 = mean over the T frames of every utterance. */
int ma_time_mean_bf16(const void* x, int64_t ldx, int64_t batch, int64_t T, int32_t halo, int32_t C, void* out,
                      ma_stream_t stream);
/* SE excitation on the squeezed vector (ecapatdnn.py:150-156) in one launch: gate (batch, C) bf16 =
 * sigmoid(W2 relu(W1 mean + b1) + b2), mean (batch, C) bf16, W1 (S, C) / W2 (C, S) bf16 row-major, float32 biases.
 * C = 512 or 1024 and S <= 128 (a multiple of 8), else MA_ERR_UNSUPPORTED (callers then run two ma_gemm_bf16). */
int ma_se_gate_bf16(const void* mean, const void* W1, const float* b1, const void* W2, const float* b2, void* gate, int64_t batch,
                    int32_t C, int32_t S, ma_stream_t stream);
/* The whole SE block behind a SERes2Net block's tdnn2 in one launch (ecapatdnn.py:150-157, 246): squeeze + excitation + scale + the
 * block's residual:  out[b, t, :] = x[b, t, :] * sigmoid(W2 relu(W1 mean_t(x[b]) + b1) + b2) + residual[b, t, :]  on the T frames, zeros
 * on the 2 halo frames of every utterance (= ma_time_mean_bf16 + ma_se_gate_bf16 + ma_se_apply_bf16, same rounding points).
 * C = 512 or 1024, S a multiple of 16 in 16 .. 128, 16-byte aligned rows, else MA_ERR_UNSUPPORTED (callers then run the three). */
int ma_se_block_bf16(const void* x, int64_t ldx, const void* W1, const float* b1, const void* W2, const float* b2, const void* residual,
                     int64_t ldr, void* out, int64_t ldo, int64_t batch, int64_t T, int32_t halo, int32_t C, int32_t S,
                     ma_stream_t stream);
/* out (M, N) float32 = a (M, K) bf16 @ W (N, K)^T + bias for few rows (the embedding Linear on the pooled statistics,
 * ecapatdnn.py:429-431): 16 x 16 output tiles, K split over the 8 waves of a workgroup.  M % 16, N % 16, K % 3072 == 0, else
 * MA_ERR_UNSUPPORTED (callers then run ma_gemm_bf16). */
int ma_linear_small_bf16(const void* a, int64_t lda, const void* W, int64_t ldw, const float* bias, float* out, int64_t ldo, int64_t M,
                         int64_t N, int64_t K, ma_stream_t stream);
/* SE excite + block residual (ecapatdnn.py:156, 246): out = gate[b, c] * x + residual on the T frames, 0 on halo frames. */
int ma_se_apply_bf16(const void* x, int64_t ldx, const void* gate, const void* residual, int64_t ldr, void* out,
                     int64_t ldo, int64_t batch, int64_t T, int32_t halo, int32_t C, ma_stream_t stream);
/* Attentive statistics pooling (ecapatdnn.py:284-308) + the BatchNorm behind it in affine form (ecapatdnn.py:427):
 * w = softmax over T of logits[:, c]; mean = sum w x; std = sqrt(clip(sum w (x - mean)^2, eps));
 * out (batch, 2C) bf16 = (mean | std) * bn_scale + bn_shift (bn_* have 2C entries). */
int ma_asp_pool_bf16(const void* logits, int64_t ldl, const void* x, int64_t ldx, int64_t batch, int64_t T, int32_t halo,
                     int32_t C, float eps, const float* bn_scale, const float* bn_shift, void* out, ma_stream_t stream);
/* The same with the logits computed in the kernel (ecapatdnn.py:296-303: logits = a1 Wc^T + bias_c over att = 128 attention
 * channels, a1 = tanh(tdnn(...)) (batch (T + 2 halo), att) bf16, Wc (C, att) bf16 row-major): one launch, no logits in memory,
 * float32 logits.  bias_c is not an argument: a per-channel constant over the frames cancels in the softmax over the frames.
 * MA_ERR_UNSUPPORTED unless att == 128, C % 256 == 0 and 16-byte aligned rows (callers then run ma_gemm_bf16 + ma_asp_pool_bf16). */
int ma_asp_fused_bf16(const void* a1, int64_t lda, const void* Wc, const void* x, int64_t ldx, int64_t batch,
                      int64_t T, int32_t halo, int32_t C, int32_t att, float eps, const float* bn_scale, const float* bn_shift,
                      void* out, ma_stream_t stream);

/* ---- post-processing around the feature kernels (mindaudio/data/features.py, spectrum.py, compute_cmvn_stats.py) --- */

/* features.compute_deltas (features.py:158-193): x (rows, T) float32, n = (win_length - 1) / 2,
 * out[t] = sum_{j=1..n} j (x[t+j] - x[t-j]) / (n (n+1) (2n+1) / 3) with the time axis padded by `pad_mode`. */
int ma_compute_deltas_f32(const float* x, int64_t rows, int64_t T, int32_t win_length, int32_t pad_mode, float* out,
                          ma_stream_t stream);
/* features.context_window (features.py:64-155): x (batch, F, T) -> out (batch, F*(left+right+1), T),
 * out[b, f*cs + k, t] = x[b, f, t + k + max(right-left, 0) - max(left, right)], zero outside [0, T). */
int ma_context_window_f32(const float* x, int64_t batch, int32_t F, int64_t T, int32_t left, int32_t right, float* out,
                          ma_stream_t stream);
/* DCT step of features.mfcc (features.py:339-356): out (batch, n_mfcc, T) = dct^T (n_mfcc, n_mels) . x (batch, n_mels, T). */
int ma_dct_f32(const float* x, int64_t batch, int32_t n_mels, int64_t T, const float* dct, int32_t n_mfcc, float* out,
               ma_stream_t stream);
/* spectrum.magphase (spectrum.py:701-735) on n complex64 values: mag = |z|^power, phase = z / |z| (1+0i at zero; phase
 * may be NULL: complex_norm). */
int ma_magphase_f32(const float* z, int64_t n, float power, float* mag, float* phase, ma_stream_t stream);
/* spectrum.magphase(iscomplex=False) (spectrum.py:732-735 -> MindSpore Magphase) on n (re, im) float pairs: mag = |z|^power,
 * angle = atan2(im, re). */
int ma_magphase_angle_f32(const float* z, int64_t n, float power, float* mag, float* angle, ma_stream_t stream);
/* op 0: out = a * x + b; op 1: out = b * ln(x + a) (features.py:343-344 log-mel: a = 1e-6, b = 1).  In place allowed. */
int ma_pointwise_f32(const float* x, int64_t n, int32_t op, float a, float b, float* out, ma_stream_t stream);
/* spectrum.frame (spectrum.py:281-304): x (batch, n) float32 or float64 (row stride ldx) -> out (batch, frame_length, num_frame)
 * float64 (the reference allocates np.zeros: float64 whatever the input), num_frame = (n - frame_length) / hop + 1,
 * out[b][i][t] = x[b][i + t * hop].  MA_ERR_HOP if hop < 1 (spectrum.py:295-296). */
int ma_frame_f64(const void* x, int32_t x_is_f64, int64_t batch, int64_t n, int64_t ldx, int32_t frame_length, int32_t hop,
                 double* out, ma_stream_t stream);
/* compute_cmvn_stats.py:45-60 on a padded feature batch x (batch, T, F) float32 with frames[b] valid rows:
 * stats (2, F) float64 += per-feature sum and sum of squares (F <= 256; the frame count is the host's sum(frames)). */
int ma_cmvn_stats_f64(const float* x, const int32_t* frames, int64_t batch, int64_t T, int32_t F, double* stats,
                      ma_stream_t stream);

/* spectrum.istft (spectrum.py:346-474): spec (batch, 1 + n_fft/2, frames_total) complex64 as ma_stft_f32 writes it (frame index
 * contiguous); the first n_frames frames are inverted (the reference trims them when `length` is given, :418-423), multiplied by
 * `window` (n_fft floats: get_window(fftbins=True) centred in n_fft, :411-415), overlap-added every `hop` samples and divided
 * by the window sum-square where that exceeds 1e-9 (:448-459).  out[b, i] = sample i + start of the overlap-added signal
 * (start = n_fft/2 when center, :461-472), zeros past its end.  Even n_fft <= 4096.
 * workspace >= ma_istft_workspace_bytes (the time-domain frames). */
int64_t ma_istft_workspace_bytes(int64_t batch, int64_t n_frames, int32_t n_fft);
int ma_istft_f32(const float* spec, int64_t batch, int32_t n_fft, int64_t frames_total, int64_t n_frames, int32_t hop,
                 const float* window, int32_t start, float* out, int64_t out_len, void* workspace, int64_t workspace_bytes,
                 ma_stream_t stream);

/* ---- on-device speed perturbation (examples/conformer/dataset.py:398-406 -> mindaudio/data/processing.py:132-176) ----------
 * resample(res_type="fft") = scipy.signal.resample over the whole utterance: out[b, :n_out[b]] = irfft(Y, n_out[b]) * n_out / n_in
 * with Y the rfft of x[b, :n_in[b]] truncated / zero-padded (Nyquist bin doubled or halved when min(n_in, n_out) is even);
 * out[b, n_out[b]:max_out] = 0.  Any lengths (Bluestein on a power-of-two length ma_resample_fft_length(max_in, max_out)
 * <= 2^23); n_in / n_out are device int32 arrays; workspace >= ma_resample_fft_workspace_bytes. */
int64_t ma_resample_fft_length(int64_t max_in, int64_t max_out);
int64_t ma_resample_fft_workspace_bytes(int64_t batch, int64_t max_in, int64_t max_out);
int ma_resample_fft_f32(const float* x, int64_t ldx, const int32_t* n_in, const int32_t* n_out, int64_t batch, int64_t max_in,
                        int64_t max_out, float* out, int64_t ldo, void* workspace, int64_t workspace_bytes,
                        ma_stream_t stream);
/* The power-of-two complex64 FFT underneath (Stockham autosort, LDS super-passes): `batch` signals of length L = 2^11 .. 2^26 in
 * `data`, scratch `tmp` of the same size; *result = whichever of the two holds the (unnormalised) transform. */
int ma_fft_pow2_c32(void* data, void* tmp, int64_t batch, int64_t L, int32_t inverse, void** result, ma_stream_t stream);

/* ---- batch assembly of the training loop (examples/conformer/dataset.py:536-656) -------------------------- */

/* len(range(max_src_len)[:-2:2][:-2:2]): width of xs_masks after the two stride-2 slicings (dataset.py:625). */
int32_t ma_subsampled_mask_len(int32_t max_src_len);

/*
 * Label and mask columns of CollateFunc.__call__ (dataset.py:570-642) for utterances already sorted by the host
 * (np.argsort(lengths)[::-1], dataset.py:484) — one launch, bit-exact:
 *   tokens   device int32, all label ids of the batch back to back; tok_off (batch+1) int32 offsets
 *   xs_lengths (batch) int32 feature frames per utterance
 *   ys_pad (batch, L) pad -1; ys_in_pad / r_ys_in_pad (batch, L+1) pad eos; ys_out_pad / r_ys_out_pad (batch, L+1)
 *   pad -1 (pad_sequence truncates over-long sequences, common.py:44); L = max_tgt_len
 *   xs_masks (batch, 1, T2) float32, T2 = ma_subsampled_mask_len(max_src_len); ys_masks (batch, 1, L+1),
 *   ys_sub_masks (batch, L+1, L+1) float32; ys_lengths (batch) int32
 *   xs_chunk_masks bool bytes: (batch, 1, T2) when chunk_size == 0 (add_optional_chunk_mask's pass-through,
 *   mask.py:270), else (batch, T2, T2) = masks & subsequent_chunk_mask(T2, chunk_size, num_left_chunks)
 *   (mask.py:154-199, 252-268; num_left_chunks < 0: all left chunks).
 */
int ma_collate_asr_i32(const int32_t* tokens, const int32_t* tok_off, const int32_t* xs_lengths, int32_t batch,
                       int32_t sos, int32_t eos, int32_t max_tgt_len, int32_t max_src_len, int32_t chunk_size,
                       int32_t num_left_chunks, int32_t* ys_pad, int32_t* ys_in_pad, int32_t* ys_out_pad,
                       int32_t* r_ys_in_pad, int32_t* r_ys_out_pad, float* xs_masks, float* ys_sub_masks,
                       float* ys_masks, int32_t* ys_lengths, uint8_t* xs_chunk_masks, ma_stream_t stream);

/* The loader's padded wave matrix on the device (round 6; dataset.py:386-406, 563-569: read -> [speed_perturb] -> waveform * 2^15 ->
 * zero-padded batch): dst (rows, ld_dst) float32, dst[r][i] = source(r)[i] for i < lengths[r], 0 up to n_dst.  source(r) = row
 * src_row[r] of `pcm` (kind[r] == 0: the files' 16-bit samples as floats = wave / 2^15 * 2^15 exactly) or of `y` (kind[r] == 1:
 * float32 rows, e.g. what ma_resample_fft_f32 made of the perturbed utterances).  All index arrays int32 on the device. */
int ma_wave_rows_f32(const int16_t* pcm, int64_t ld_pcm, const float* y, int64_t ld_y, const int32_t* src_row, const int32_t* kind,
                     const int32_t* lengths, int64_t rows, float* dst, int64_t ld_dst, int64_t n_dst, ma_stream_t stream);

/*
 * CollateFunc.spec_aug (dataset.py:493-534) on the padded batch xs (batch, max_frames, n_freq) float32, in place.
 * The host draws the intervals with the reference's `random` call order; t_intervals (batch, n_t, 2) /
 * f_intervals (batch, n_f, 2) int32 hold [start, end) per mask, an empty interval for a mask the 20 % coin skipped.
 * Frequency masks cover the utterance's xs_lengths[b] valid frames.
 */
int ma_spec_aug_f32(float* xs, int64_t batch, int64_t max_frames, int32_t n_freq, const int32_t* xs_lengths,
                    const int32_t* t_intervals, int32_t n_t, const int32_t* f_intervals, int32_t n_f,
                    ma_stream_t stream);

/* ---- training step (mindaudio/utils/train_one_step.py:13-48 around examples/conformer/asr_model.py) -------------
 * Memory-bound backward pieces and the optimizer; the matmuls of the backward pass reuse ma_gemm_bf16
 * (dX = dY . W on a transposed weight copy) and ma_gemm_bf16_splitk_f32 (dW = dY^T . X on transposed activations). */

/* out (M, N) float32 (+)= alpha * A (M, K) . W (N, K)^T with the contraction split across workgroups (weight
 * gradients: small outputs, K = batch*time): every split writes its partial product to `workspace`
 * (>= ma_gemm_splitk_workspace_bytes), a second kernel sums the splits in a fixed order (deterministic).  K % 64 == 0. */
int64_t ma_gemm_splitk_workspace_bytes(int64_t M, int64_t N, int64_t K);
int ma_gemm_bf16_splitk_f32(const void* A, int64_t lda, const void* W, int64_t ldw, float* out, int64_t ldo,
                            int64_t M, int64_t N, int64_t K, float alpha, int32_t accumulate, void* workspace,
                            int64_t workspace_bytes, ma_stream_t stream);

/* out (Mo_store, No) float32 (+)= alpha * A^T . B for ROW-major A (Kc, Mo), B (Kc, No) bf16: dW = dY^T . X straight from
 * the activations (no transposed copies; LDS transpose-reads feed the MFMAs).  Rows i >= Mo_store of the product are
 * not stored (zero-padded vocabulary columns).  colsum (Mo_store) float32, optional: += column sums of A (bias
 * gradient; one partial vector per split, added in split order: deterministic).  Mo, No, lda, ldb multiples of 8;
 * workspace >= ma_gemm_tn_workspace_bytes(Mo, No, Kc) = splits * Mo * (No + 1) * 4 with splits = ma_gemm_tn_splits(Mo, No, Kc). */
int64_t ma_gemm_tn_workspace_bytes(int64_t Mo, int64_t No, int64_t Kc);
int32_t ma_gemm_tn_splits(int64_t Mo, int64_t No, int64_t Kc);
int ma_gemm_tn_bf16_f32(const void* A, int64_t lda, const void* B, int64_t ldb, float* out, int64_t ldo, int64_t Mo,
                        int64_t No, int64_t Kc, int64_t Mo_store, float alpha, int32_t accumulate, float* colsum,
                        void* workspace, int64_t workspace_bytes, ma_stream_t stream);
/* The two halves of ma_gemm_tn_bf16_f32 apart, so that the split sums of many products leave in ONE launch (the training step:
 * 8 weight gradients per block, each followed by a launch-bound 6.6 us reduction otherwise).
 * ma_gemm_tn_partial_bf16 writes the split-K partial products [splits][Mo_store][No] float32 into `partial`
 * (>= ma_gemm_tn_workspace_bytes(Mo, No, Kc) bytes, splits = ma_gemm_tn_splits(Mo, No, Kc)) and, with_colsum != 0, the partial
 * column sums of A [splits][Mo_store] behind them (float offset splits * Mo_store * No).
 * ma_reduce_splits_batch_f32: items / block_item are DEVICE arrays; item i adds its `splits` partial matrices of `mn` elements
 * (`pstride` floats apart; 0 = mn) in order and stores out[m][n] = (accumulate ? out : 0) + alpha * sum with row length N and row
 * stride ldo; workgroup b handles elements [1024 (b - first_block), + 1024) of item block_item[b] - or, for a "tall" item
 * (accumulate bit 1 set: hundreds of partials of a few hundred elements), elements [16 (b - first_block), + 16), the partials spread
 * over 64 thread groups.  Every parameter-gradient
 * reduction of the training step (weight-gradient splits, bias / LayerNorm / BatchNorm / depthwise / positional-bias partials)
 * goes through this one kernel, one launch per Conformer block: fixed summation order, no float atomics. */
typedef struct ma_reduce_item {
  const float* part;
  float* out;
  int64_t mn, ldo;
  int32_t N, splits;
  float alpha;
  int32_t accumulate;
  int32_t first_block, pstride;
} ma_reduce_item_t;
int ma_gemm_tn_partial_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, int64_t Mo, int64_t No, int64_t Kc,
                            int64_t Mo_store, int32_t with_colsum, void* partial, int64_t partial_bytes, ma_stream_t stream);
int ma_reduce_splits_batch_f32(const ma_reduce_item_t* items, const int32_t* block_item, int32_t n_blocks, ma_stream_t stream);
/* ma_gemm_tn_partial_bf16 for a list of products in ONE launch per eight of them (`items` is a HOST array; the arguments of one
 * ma_gemm_tn_partial_bf16 call each).  The eight weight gradients of a Conformer block are issued together (on their own stream):
 * one grid instead of eight.  Same workgroups, same partials as the separate calls, bit for bit. */
typedef struct ma_tn_item {
  const void* A;
  const void* B;
  void* partial;
  int64_t lda, ldb, Mo, No, Kc, Mo_store, partial_bytes;
  int32_t with_colsum, reserved;
} ma_tn_item_t;
int ma_gemm_tn_partial_group_bf16(const ma_tn_item_t* items, int32_t n, ma_stream_t stream);

/* Weight-gradient products WITHOUT split-K (round 4): out (Mo, No) float32 = A^T B, colsum (Mo, may be NULL) = column sums of A,
 * for up to ma_gemm_tn_direct_max_items() products in ONE grid of 256 x 256 tiles, each tile with the full contraction - no partial
 * products, no reduction pass; results are STORED (not accumulated).  `items` is a HOST array.  The training engine issues the
 * products of several Conformer blocks together (39 tiles per block: six blocks fill the chip).  Needs Mo % 256 == No % 256 == 0,
 * lda % 8 == ldb % 8 == ldo % 4 == 0 and 16-byte aligned pointers: MA_ERR_UNSUPPORTED otherwise (the caller falls back to
 * ma_gemm_tn_partial_group_bf16).  Gradients of mindaudio/models/layers/dense.py:16-62 under train_one_step.py:36-41. */
typedef struct ma_tn_direct_item {
  const void* A;  /* (Kc, >= Mo) bf16, row stride lda */
  const void* B;  /* (Kc, >= No) bf16, row stride ldb */
  float* out;     /* (Mo, No), row stride ldo */
  float* colsum;  /* (Mo) or NULL */
  int64_t lda, ldb, ldo;
  int32_t Mo, No, Kc, reserved;
} ma_tn_direct_item_t;
int32_t ma_gemm_tn_direct_max_items(void);
int ma_gemm_tn_direct_group_bf16(const ma_tn_direct_item_t* items, int32_t n, ma_stream_t stream);



/* ---- training forms of the packed dense layers: the layer's element-wise neighbours ride in the epilogue ---------------------
 * One struct describes them (NULL / 0 switch a term off):
 *   mode 1  w_1 forward:   out = u = bf16(acc + bias), out2 = h = bf16(dropout(swish(u)))   (positionwise_feed_forward.py:44-46)
 *   mode 2  w_1 backward:  out = du = bf16(bf16(acc) * swish'(u) * keep / (1 - p)), u = aux (M, N) bf16; acc = dy . W_2
 *   mode 3  branch joins (N = 256): z = bf16((acc + bias) * row_scale[m]); out (float32) = residual + alpha * dropout(z)
 *           (models/conformer.py:109-151); then optionally ln_out = LayerNorm(out; gamma1, beta1) * ln_row_scale[m] (bf16 or
 *           float32), or - with gamma2 - ln_mid (float32) = LayerNorm(out; gamma1, beta1) and ln_out = LayerNorm(ln_mid; gamma2,
 *           beta2): norm_final of a block chained with the LayerNorm that consumes it (:153-156, 109-110, 253-254)
 *   mode 4  plain:         out = bf16(acc + bias)                                             (input gradients)
 * Dropout = the counter-based mask of ma_dropout_add_f32 / ma_act_dropout_*: element index m * N + n of site (seed, salt), so the
 * fused and the un-fused launches of one site agree bit for bit (u, h, du are bit-identical to the un-fused launches). */
typedef struct ma_train_epilogue {
  int32_t mode;
  int32_t ln_out_bf16;
  const float* bias;
  const void* aux;
  int64_t ld_aux;
  void* out2;
  int64_t ldo2;
  const float* residual;
  int64_t ldr;
  const float* row_scale;
  float alpha;
  float p;
  uint32_t seed, salt;
  const float *ln_gamma1, *ln_beta1, *ln_gamma2, *ln_beta2, *ln_row_scale;
  void* ln_out;
  float* ln_mid;
  int64_t ld_ln, ld_mid;
  float ln_eps;
  int32_t act;     /* modes 1 / 2: 0 or 1 = Swish (layers/swish.py, the Conformer blocks), 2 = ReLU (the TransformerDecoder's
                      feed-forward, models/conformer.py:430-470); was `reserved` (0) until round 6 */
} ma_train_epilogue_t;
/* K = 256 layers on the packed weight of ma_gemm_k256_pack_bf16 (N % 256 == 0); out bf16 (modes 1, 2, 4) or float32 (mode 3). */
int ma_gemm_k256_train_bf16(const void* A, int64_t lda, const void* packed, void* out, int64_t ldo, int64_t M, int64_t N,
                            const ma_train_epilogue_t* epi, ma_stream_t stream);
/* N = 256 layers with a long contraction (K % 64 == 0) on the packed weight of ma_gemm_rows_pack_bf16: modes 3, 4 and 5.
 * mode 5 (round 4) = an input-gradient product + the BACKWARD of the LayerNorm in front of the layer + the next branch's dropout
 * backward in one launch (models/conformer.py:109-151 differentiated): dy = bf16(acc) * row_scale; with x = residual (ldr),
 * gamma = ln_gamma1, eps = ln_eps: out (float32, IN PLACE: the residual-stream gradient g) += dLN/dx(dy); optional ln_out (bf16,
 * ld_ln) = dropout(g * alpha * ln_row_scale) with (p, seed, salt); ln_mid = per-workgroup partial (dgamma | dbeta) vectors,
 * ma_gemm_rows_train_parts(M) x 512 floats.  Same arithmetic as ma_layernorm_bwd_next_f32 behind ma_gemm_rows_train_bf16 mode 4,
 * row sums in another order. */
int32_t ma_gemm_rows_train_parts(int64_t M);
int ma_gemm_rows_train_bf16(const void* A, int64_t lda, int64_t M, int64_t K, const void* packed, void* out, int64_t ldo,
                            const ma_train_epilogue_t* epi, ma_stream_t stream);
/* A branch join (mode 3 without the chained second LayerNorm; N = 256) behind a long contraction over FEW rows (round 6: the
 * TransformerDecoder's w_2, models/conformer.py:430-470 + 501-530: 1 240 rows x K = 2048 - 40 output tiles would walk 32 K-tiles each
 * on 40 of the 256 CUs): the product of row-major A (M, K) and W (256, K) [the weight as the reference stores it, no packed copy]
 * is split over K like ma_gemm_bf16_splitk_f32 (`workspace` >= ma_gemm_splitk_workspace_bytes(M, 256, K)), and the launch that adds
 * the splits in their fixed order carries the join: out (float32) = residual + alpha * dropout(bf16((sum + bias) * row_scale)),
 * ln_out = LayerNorm(out; ln_gamma1, ln_beta1) * ln_row_scale.  `out` is bit-identical to ma_gemm_bf16_splitk_f32 + bias + a bf16
 * rounding + ma_dropout_add_f32, ln_out within one bf16 ulp of ma_layernorm_f32 of it (tests/test_train_kernels_gpu.py); two
 * launches instead of four. */
int ma_gemm_bf16_splitk_join_f32(const void* A, int64_t lda, const void* W, int64_t ldw, float* out, int64_t ldo, int64_t M,
                                 int64_t N, int64_t K, const ma_train_epilogue_t* epi, void* workspace, int64_t workspace_bytes,
                                 ma_stream_t stream);
/* The whole position-wise feed-forward module of a Conformer block in TRAINING mode, one launch each way (round 4; d_model = 256,
 * hidden % 256 == 0, `packed` = ma_ffn_pack_weights_bf16 - the evaluation forward's format).
 * Forward:
 *   u (M, hidden) bf16 = a W1^T + b1;  h (M, hidden) bf16 = dropout(swish(a W1^T + b1)) with (p_hidden, seed_hidden, salt_hidden)
 *   [both are the backward pass's tape, row stride ldu];  out (M, 256) float32 = the join of ma_gemm_rows_train_bf16 mode 3 on
 *   h W2^T (`join`: bias = b2, residual, alpha, the join's dropout site, LayerNorm / LayerNorm chain outputs).
 *   tape_derivative != 0: u receives gk = bf16(swish'(a W1^T + b1) * keep / (1 - p_hidden)) instead - all the backward pass needs of u.
 * positionwise_feed_forward.py:33-46 + models/conformer.py:109-112, 147-156.  Against ma_gemm_k256_train_bf16 mode 1 followed by
 * ma_gemm_rows_train_bf16 mode 3: the same dropout masks element for element; the bias enters the float32 accumulation of u first
 * instead of last, Swish is taken of the float32 pre-activation instead of its bf16 rounding, and the second product sums the
 * hidden units in another order (tests/test_train_kernels_gpu.py carries the tolerances).
 * Backward (`packed_t` = ma_ffn_pack_weights_bf16 of (W2^T (hidden, 256), W1^T (256, hidden)); gk from the forward launch):
 *   du (M, hidden) bf16 = bf16(dy W2) * gk   [stored: the operand of w_1's weight gradient];  da = du W1 feeds the LayerNorm backward
 *   of ma_gemm_rows_train_bf16 mode 5 (`lnbwd`: residual = the LayerNorm's input x, ln_gamma1, g in place, ln_mid = per-workgroup
 *   (dgamma | dbeta) partials, ma_ffn_train_parts(M) x 512 floats, optional ln_out = the next branch's dropout backward).
 *   Against ma_gemm_k256_train_bf16 mode 2 + ma_gemm_rows_train_bf16 mode 5: swish' comes from the forward's float32 pre-activation
 *   through one bf16 rounding (gk) instead of from the bf16 u.
 *   `chain` (may be NULL; `lnbwd` then has no ln_out): a SECOND LayerNorm backward on the finished rows, for the LayerNorm whose
 *   output the rows of g are - residual = its input x2, ln_gamma1 = its weight, ln_mid = its partials: g is REPLACED by
 *   dLN2/dx(g) (not accumulated), ln_out = dropout(g * alpha * ln_row_scale).  In the Conformer block this is norm_ff_macaron's
 *   backward of block l followed by norm_final's of block l - 1 (models/conformer.py:109-112, 153-156) without the round trip of g
 *   through HBM and the launch of ma_layernorm_bwd_next_f32 between them.
 * Both need M * ldu < 2^31 elements.  ma_ffn_train_rows() = rows per workgroup (48).
 * Forward without a tape (a training-mode forward that no backward pass follows): ldu = 0, u and h = two scratch areas of
 * 2 * hidden bytes each - every row's pieces of a hidden block are stored onto the same 64 bytes there (never read; they stay in
 * the L2), everything else as above. */
int32_t ma_ffn_train_rows(void);
int32_t ma_ffn_train_parts(int64_t M);
int ma_ffn_train_bf16(const void* a, int64_t lda, int64_t M, int32_t hidden, const void* packed, const float* b1, void* u, void* h,
                      int64_t ldu, int32_t tape_derivative, float p_hidden, uint32_t seed_hidden, uint32_t salt_hidden, float* out,
                      int64_t ldo, const ma_train_epilogue_t* join, ma_stream_t stream);
int ma_ffn_train_bwd_bf16(const void* dy, int64_t ldy, int64_t M, int32_t hidden, const void* packed_t, const void* gk, void* du,
                          int64_t ldu, float* g, int64_t ldg, const ma_train_epilogue_t* lnbwd, const ma_train_epilogue_t* chain,
                          ma_stream_t stream);
/* Fragment packing of a list of weights in ONE launch (the training step re-packs every layer's weights after the optimizer):
 * items / block_item are DEVICE arrays; kind 0 = ma_gemm_k256_pack_bf16 layout (K = 256), kind 1 = ma_gemm_rows_pack_bf16 layout
 * (N = 256), kind 2 / 3 = the W1 (N = hidden, K = 256) / W2 (N = 256, K = hidden) half of ma_ffn_pack_weights_bf16's format (both
 * halves of a module share one destination); workgroup b packs 16-byte pieces [256 (b - first_block), + 256) of item
 * block_item[b]. */
typedef struct ma_pack_item {
  const void* src;
  void* dst;
  int64_t ld;
  int32_t N, K, kind, first_block;
} ma_pack_item_t;
int64_t ma_pack_item_pieces(int32_t kind, int64_t N, int64_t K);
int ma_pack_batch_bf16(const ma_pack_item_t* items, const int32_t* block_item, int32_t n_blocks, ma_stream_t stream);

/* Weight gradient of the 3x3 stride-2 valid Conv2d of the subsampling layer (layers/subsampling.py:42) as the same TN
 * GEMM with an implicit im2col B operand: dw (Cout, 9C) float32 += dy^T . im2col(act), dbias (Cout) += column sums of dy.
 * dy (batch*Ho*Wo, Cout) bf16 row stride ld_dy; act (batch, H, Wd, C) NHWC bf16; C % 128 == 0.
 * workspace >= ma_gemm_tn_workspace_bytes(Cout, 9C, batch*Ho*Wo); with >= ma_conv2d_3x3s2_dw_workspace_bytes(batch*Ho*Wo, C, Cout)
 * bytes and C % 256 == Cout % 256 == 0 the product runs on 256 x 256 tiles (round 4: half the operand bytes per flop). */
int64_t ma_conv2d_3x3s2_dw_workspace_bytes(int64_t rows, int64_t C, int64_t Cout);
int ma_conv2d_3x3s2_dw_bf16(const void* dy, int64_t ld_dy, const void* act, int64_t batch, int64_t H, int64_t Wd, int64_t C,
                            int64_t Cout, float* dw, float* dbias, void* workspace, int64_t workspace_bytes,
                            ma_stream_t stream);

/* out[c][r] = in[r][c] (bf16); columns r in [rows, ld_out) of `out` are not written (keep them zero to use the
 * result as a K-padded GEMM operand).  colsum (cols) float32, optional: += column sums of `in` (bias gradients). */
int ma_transpose_bf16(const void* in, int64_t ld_in, int64_t rows, int64_t cols, void* out, int64_t ld_out,
                      float* colsum, ma_stream_t stream);

/* The same for a list of matrices in ONE launch (the transposed bf16 weight copies of the training step: 100 matrices per
 * step, each of them a launch-bound 4 us on its own).  `items` and `block_item` are DEVICE arrays: block_item[b] = index of the
 * item whose 64 x 64 tile workgroup b transposes, items[i].first_block = index of its first workgroup; tiles of an item are
 * numbered row-tile major: tile = (b - first_block), r0 = 64 * (tile / tiles_c), c0 = 64 * (tile % tiles_c).  All bases 16-byte
 * aligned, ld_in / ld_out / cols multiples of 8. */
typedef struct ma_transpose_item {
  const void* in;
  void* out;
  int64_t ld_in, ld_out;
  int32_t rows, cols;
  int32_t first_block, tiles_c;
} ma_transpose_item_t;
int ma_transpose_batch_bf16(const ma_transpose_item_t* items, const int32_t* block_item, int32_t n_blocks, ma_stream_t stream);

/* Backward of ma_layernorm_f32 (layers/layernorm.py:53-60): g (+)= dL/dx, dgamma/dbeta (D) float32 += the sum of the
 * per-workgroup partials in a fixed order (run-to-run deterministic).  dy bf16 or float32; row_scale as in the forward; D = 256,
 * 512, 768 or 1024 (round 6: the reference's constructor takes any d_model, models/conformer.py:293-313).
 * workspace >= ma_layernorm_bwd_parts(rows) * 2 D * 4 bytes: [parts][dgamma (D) | dbeta (D)].  dgamma == NULL: the partials are
 * left in `workspace` for the caller's ma_reduce_splits_batch_f32 (the training step sums a block's partials in one launch). */
int32_t ma_layernorm_bwd_parts(int64_t rows);
int ma_layernorm_bwd_f32(const float* x, int64_t ldx, int64_t rows, int64_t D, const float* gamma, float eps,
                         const float* row_scale, const void* dy, int64_t ldy, int32_t dy_bf16, float* g, int64_t ldg,
                         int32_t accumulate, float* dgamma, float* dbeta, void* workspace, int64_t workspace_bytes,
                         ma_stream_t stream);
/* The same, and on every finished row of g the NEXT branch's ma_dropout_bwd_bf16 (the residual stream's gradient enters the
 * branch in front: dy_next (rows, 256) bf16 = alpha_next * keep / (1 - p_next) * g * row_scale_next[r], site (seed, salt_next)). */
int ma_layernorm_bwd_next_f32(const float* x, int64_t ldx, int64_t rows, int64_t D, const float* gamma, float eps,
                              const float* row_scale, const void* dy, int64_t ldy, int32_t dy_bf16, float* g, int64_t ldg,
                              int32_t accumulate, float* dgamma, float* dbeta, void* workspace, int64_t workspace_bytes,
                              void* dy_next, int64_t ld_next, float alpha_next, const float* row_scale_next, float p_next,
                              uint32_t seed, uint32_t salt_next, ma_stream_t stream);
/* Scratch for the two-stage parameter-gradient reductions of ma_layernorm_bwd_f32, ma_convmid_bwd_bf16 and
 * ma_subsample_conv1_dw_f32 (per-workgroup partial sums, then a fixed-order sum: no contended atomics). */
int64_t ma_train_reduce_workspace_bytes(void);

/* h = dropout(act(u)) between w_1 and w_2 (positionwise_feed_forward.py:33-46), bf16, n elements; act: 1 swish
 * (encoder), 2 relu (decoder, conformer.py:521).  The keep mask is a pure function of (seed, salt, element index) and is
 * regenerated by the backward: du = dh * keep/(1-p) * act'(u). */
int ma_act_dropout_fwd_bf16(const void* u, void* h, int64_t n, int32_t act, float p, uint32_t seed, uint32_t salt,
                            ma_stream_t stream);
int ma_act_dropout_bwd_bf16(const void* u, const void* dh, void* du, int64_t n, int32_t act, float p, uint32_t seed,
                            uint32_t salt, ma_stream_t stream);

/* x (rows, cols) float32 = xin + alpha * dropout(y) (models/conformer.py:109-151 branch joins; xin may be x, or NULL for
 * no residual term: the dropout of layers/embedding.py:86-87); y bf16 or float32.  Backward: dy (bf16) = alpha * keep/(1-p) * g * row_scale[r]. */
int ma_dropout_add_f32(float* x, int64_t ldx, const float* xin, int64_t ldxin, const void* y, int64_t ldy, int32_t y_bf16,
                       int64_t rows, int64_t cols, float alpha, float p, uint32_t seed, uint32_t salt, ma_stream_t stream);
int ma_dropout_bwd_bf16(const float* g, int64_t ldg, void* dy, int64_t ldy, int64_t rows, int64_t cols, float alpha,
                        const float* row_scale, float p, uint32_t seed, uint32_t salt, ma_stream_t stream);

/* Convolution module in training mode (layers/convolution.py:83-129), between the two pointwise GEMMs:
 *   ma_convmid_fwd_train   z (B*T, C) float32 = depthwise_k(glu(y)) + bias, y (B*T, 2C) bf16; sums = one partial vector
 *                          (sum z | sum z^2) of 2C floats per workgroup, ma_convmid_fwd_train_parts(batch, T, C) of them
 *   ma_bn_finalize_f32     adds the `nparts` partial vectors in a fixed order; stats = (mean[C], rstd[C]) of the B*T rows
 *                          (biased variance); running statistics updated with momentum and the unbiased variance (nn.BatchNorm1d)
 *   ma_bn_swish_fwd_bf16   out = swish(gamma * (z - mean) * rstd + beta) bf16
 *   ma_bn_swish_bwd_f32    dz (float32) from dout (bf16): Swish', then the BatchNorm backward; dsum (2C) float32 =
 *                          (sum dn | sum dn zhat), stored; d_gamma / d_beta (C, optional) += the parameter gradients;
 *                          workspace >= 1024 * 2C * 4 bytes (per-workgroup partials, summed in a fixed order)
 *   ma_convmid_bwd_bf16    dy (B*T, 2C) bf16 from dz: depthwise-conv backward + GLU backward; d_dw_w (C, k), d_dw_b (C)
 *                          float32 += per-workgroup partials summed in a fixed order
 * No float atomics anywhere: two runs of a training step give bit-identical gradients. */
int32_t ma_convmid_fwd_train_parts(int64_t batch, int64_t T, int32_t C);
int ma_convmid_fwd_train(const void* y, int64_t ldy, int64_t batch, int64_t T, int32_t C, const float* dw_w,
                         int32_t ks, const float* dw_b, float* z, float* sums, ma_stream_t stream);
int ma_bn_finalize_f32(const float* sums, int32_t nparts, int32_t C, int64_t count, float eps, float momentum,
                       float* running_mean, float* running_var, float* stats, ma_stream_t stream);
int ma_bn_swish_fwd_bf16(const float* z, const float* stats, const float* gamma, const float* beta, void* out,
                         int64_t rows, int32_t C, ma_stream_t stream);
int ma_bn_swish_bwd_f32(const void* dout, const float* z, const float* stats, const float* gamma, const float* beta,
                        float* dz, int64_t rows, int32_t C, float* dsum, float* d_gamma, float* d_beta, void* workspace,
                        int64_t workspace_bytes, ma_stream_t stream);
/* (ma_convmid_bwd_*: workspace >= ma_convmid_bwd_parts(batch, T) * C * (k + 1) * 4 bytes of per-workgroup partials
 * [parts][d_dw_w (C, k) | d_dw_b (C)]; d_dw_w == NULL leaves them there for the caller's ma_reduce_splits_batch_f32.) */
int32_t ma_convmid_bwd_parts(int64_t batch, int64_t T);
int ma_convmid_bwd_bf16(const float* dz, const void* y, int64_t ldy, int64_t batch, int64_t T, int32_t C,
                        const float* dw_w, int32_t ks, void* dy, int64_t lddy, float* d_dw_w, float* d_dw_b,
                        void* workspace, int64_t workspace_bytes, ma_stream_t stream);
/* The two above with the BatchNorm backward's second stage folded into the depthwise backward's loads (round 4):
 * ma_bn_swish_bwd_stage1_f32 = ma_bn_swish_bwd_f32 without that stage (dn = dout * swish'(n) is left in `dn`, dsum / d_gamma / d_beta
 * as before); ma_convmid_bwd_bn_bf16 = ma_convmid_bwd_bf16 on dz = gamma rstd (dn - dsum[c] / N - zhat dsum[C + c] / N), N = batch * T,
 * formed element for element as the second stage forms it (same results, one launch and one float32 round trip fewer). */
int ma_bn_swish_bwd_stage1_f32(const void* dout, const float* z, const float* stats, const float* gamma, const float* beta,
                               float* dn, int64_t rows, int32_t C, float* dsum, float* d_gamma, float* d_beta, void* workspace,
                               int64_t workspace_bytes, ma_stream_t stream);
int ma_convmid_bwd_bn_bf16(const float* dn, const float* z, const float* stats, const float* gamma, const float* dsum, const void* y,
                           int64_t ldy, int64_t batch, int64_t T, int32_t C, const float* dw_w, int32_t ks, void* dy, int64_t lddy,
                           float* d_dw_w, float* d_dw_b, void* workspace, int64_t workspace_bytes, ma_stream_t stream);

/* Conv2dSubsampling4 backward (layers/subsampling.py:21-78): ReLU mask in place; transposed im2col matrix
 * (9C, ld_out >= B*Ho*Wo) of an NHWC bf16 activation (weight gradient of conv2 as a split-K GEMM); col2im + ReLU mask
 * (input gradient of conv2 from dcol (B*Ho*Wo, 9C) bf16); conv1 weight/bias gradient (C, 9) / (C) float32 +=. */
int ma_relu_bwd_bf16(void* dy, const void* y, int64_t n, ma_stream_t stream);
int ma_im2col_t_3x3s2_nhwc_bf16(const void* act, int64_t batch, int64_t H, int64_t Wd, int64_t C, void* out,
                                int64_t ld_out, ma_stream_t stream);
int ma_col2im_3x3s2_relu_bf16(const void* dcol, const void* act, int64_t batch, int64_t H, int64_t Wd, int64_t C,
                              void* dact, ma_stream_t stream);
int ma_subsample_conv1_dw_f32(const void* dact, const float* x, int64_t batch, int64_t T, int32_t idim,
                              const float* cmvn_mean, const float* cmvn_istd, int32_t C, float* dw, float* db,
                              void* workspace, int64_t workspace_bytes, ma_stream_t stream);

/* Rel-pos attention for training: the forward of ma_relpos_attention_bf16 that also writes lse (batch, heads, T)
 * float32 = log-sum-exp of the scaled, masked scores of every query row, and the backward pass
 * (layers/attention.py:182-237): from dctx (batch*T, 256) bf16 to dqkv (batch*T, 768) bf16 (dq | dk | dv),
 * dpos (T, 256) float32 with row stride ld_dpos += (summed over the batch), dbias_u / dbias_v (heads, 64) float32 +=
 * (caller zeroes the three). */
int ma_relpos_attention_train_bf16(const void* qkv, int64_t ld_qkv, const void* pos, int64_t ld_pos,
                                   const float* bias_u, const float* bias_v, const float* mask, int64_t batch,
                                   int64_t T, int32_t heads, int32_t d_k, void* ctx, int64_t ld_ctx,
                                   void* vt_workspace, int64_t vt_bytes, float* lse, ma_stream_t stream);
int64_t ma_relpos_attention_bwd_workspace_bytes(int64_t batch, int64_t T, int32_t heads, int32_t d_k);
int ma_relpos_attention_bwd_bf16(const void* qkv, int64_t ld_qkv, const void* pos, int64_t ld_pos, const float* bias_u,
                                 const float* bias_v, const float* mask, const void* ctx, int64_t ld_ctx,
                                 const void* dctx, int64_t ld_dctx, const float* lse, int64_t batch, int64_t T,
                                 int32_t heads, int32_t d_k, void* dqkv, int64_t ld_dqkv, float* dpos, int64_t ld_dpos,
                                 float* dbias_u, float* dbias_v, void* workspace, int64_t workspace_bytes,
                                 ma_stream_t stream);
/* dpos == NULL (dbias_u / dbias_v then unused): the backward leaves its partial sums in the workspace and the caller adds them with
 * ma_reduce_splits_batch_f32 (the training step: one reduction launch per block); ma_relpos_attention_bwd_layout gives their float
 * offsets: dp_part [batch][Tp][256] (sum over the batch -> dpos (T, 256)), bias_part [heads][parts_per_head][128] = (du | dv). */
int ma_relpos_attention_bwd_layout(int64_t batch, int64_t T, int32_t heads, int32_t d_k, int64_t* dp_part_off, int64_t* bias_part_off,
                                   int32_t* Tp_out, int32_t* parts_per_head);

/* The same two with a per-(query, key) mask (batch, T, T) float32 instead of the (batch, T) padding mask: the chunk masks
 * of the streaming configuration (utils/mask.py:201-271; models/conformer.py:251-252 hands them to every block). */
int ma_relpos_attention_train_qmask_bf16(const void* qkv, int64_t ld_qkv, const void* pos, int64_t ld_pos,
                                         const float* bias_u, const float* bias_v, const float* mask_qk, int64_t batch,
                                         int64_t T, int32_t heads, int32_t d_k, void* ctx, int64_t ld_ctx,
                                         void* vt_workspace, int64_t vt_bytes, float* lse, ma_stream_t stream);
int ma_relpos_attention_bwd_qmask_bf16(const void* qkv, int64_t ld_qkv, const void* pos, int64_t ld_pos, const float* bias_u,
                                       const float* bias_v, const float* mask_qk, const void* ctx, int64_t ld_ctx,
                                       const void* dctx, int64_t ld_dctx, const float* lse, int64_t batch, int64_t T,
                                       int32_t heads, int32_t d_k, void* dqkv, int64_t ld_dqkv, float* dpos, int64_t ld_dpos,
                                       float* dbias_u, float* dbias_v, void* workspace, int64_t workspace_bytes,
                                       ma_stream_t stream);

/* ---- attention-decoder branch of the hybrid loss (models/conformer.py:382-639, asr_model.py:154-186) -----------
 * Token-sized pieces; the decoder's matmuls, LayerNorms (eps 1e-12) and dropouts reuse the entry points above. */

/* nn.Embedding -> x * xscale + pe[l] -> dropout (layers/embedding.py:16-62): out (rows, D) float32, rows = batch * L,
 * token ids clamped into [0, V).  Backward: dtable (V, D) float32 += scatter of xscale * keep/(1-p) * g, every table row summed by
 * one workgroup in row order (no float atomics); D <= 1024, MA_ERR_UNSUPPORTED beyond. */
int ma_embed_posenc_f32(const int32_t* tokens, const float* table, const float* pe, int64_t rows, int32_t L, int32_t D,
                        int32_t V, float xscale, float p, uint32_t seed, uint32_t salt, float* out, ma_stream_t stream);
int ma_embed_bwd_f32(const int32_t* tokens, const float* g, int64_t rows, int32_t D, int32_t V, float xscale, float p,
                     uint32_t seed, uint32_t salt, float* dtable, ma_stream_t stream);
/* The same with a row mask (rows float32, may be NULL): rows with row_keep == 0 are skipped.  For the caller that KNOWS their
 * gradient is zero - the padded label positions of the attention decoder (add_sos_eos pads ys_in with <eos>, utils/common.py:40-88;
 * the (B, L, L) label mask keeps them out of every valid position's attention, asr_model.py:117-144): a third of the rows and one
 * token id, i.e. one workgroup's serial sum (84 -> ~20 us per cfg-4 hybrid step). */
int ma_embed_bwd_rows_f32(const int32_t* tokens, const float* g, const float* row_keep, int64_t rows, int32_t D, int32_t V,
                          float xscale, float p, uint32_t seed, uint32_t salt, float* dtable, ma_stream_t stream);

/* MultiHeadedAttention core (layers/attention.py:86-157) for Lq <= 1024 queries (walked in tiles of 32, one launch each: labels of
 * more than 31 tokens - the data set classes' default token_max_length is 200, the shipped yaml sets 30 - were refused until round 6) and Lk <= 1088 keys per (batch, head)
 * (up to 320 keys the V / K rows are staged in LDS; beyond that - the 1400 ... 3000-frame buckets of conformer.yaml, T' <= 749 -
 * the score rows take the LDS and V / K are read from L2; more keys: MA_ERR_UNSUPPORTED), d_k = 64: ctx = softmax(scale * q k^T + (mask == 0 ? -10000 : 0)) v.  q (batch*Lq, H*64) / k, v (batch*Lk, H*64) bf16
 * with row strides; mask_mode 0 none, 1 (batch, 1, Lk), 2 (batch, Lq, Lk) float32; probs (batch, H, Lq, Lk) float32 is
 * written by the forward and read by the backward (dq, dk, dv bf16 with their own row strides). */
int ma_mha_small_fwd_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                          const float* mask, int32_t mask_mode, int64_t batch, int32_t Lq, int32_t Lk, int32_t heads,
                          int32_t d_k, float scale, void* ctx, int64_t ldc, float* probs, ma_stream_t stream);
int ma_mha_small_bwd_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                          const float* probs, const void* ctx, int64_t ldc, const void* dctx, int64_t lddc, int64_t batch,
                          int32_t Lq, int32_t Lk, int32_t heads, int32_t d_k, float scale, void* dq, int64_t lddq, void* dk,
                          int64_t lddk, void* dv, int64_t lddv, ma_stream_t stream);

/* ma_mha_small_fwd_bf16 for `batch` query rows groups that share keys: query batch b reads the keys, values and the (batch, 1, Lk)
 * mask (mask_mode 1) of batch b / kv_group - k, v (batch / kv_group * Lk, ...), mask (batch / kv_group, 1, Lk); a (batch, Lq, Lk)
 * mask (mode 2) stays per query batch.  The attention rescoring's source attention: beam hypotheses against one encoder output
 * without repeating it.  batch % kv_group == 0; kv_group == 1 is ma_mha_small_fwd_bf16, bit for bit. */
int ma_mha_small_fwd_grouped_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                  const float* mask, int32_t mask_mode, int64_t batch, int32_t Lq, int32_t Lk, int32_t heads,
                                  int32_t d_k, float scale, int32_t kv_group, void* ctx, int64_t ldc, float* probs,
                                  ma_stream_t stream);

/* The same on float32 activations (the float32 validation mode of the hybrid loss; always the un-staged form). */
int ma_mha_small_fwd_x32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* mask,
                         int32_t mask_mode, int64_t batch, int32_t Lq, int32_t Lk, int32_t heads, int32_t d_k, float scale, float* ctx,
                         int64_t ldc, float* probs, ma_stream_t stream);
int ma_mha_small_bwd_x32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* probs,
                         const float* ctx, int64_t ldc, const float* dctx, int64_t lddc, int64_t batch, int32_t Lq, int32_t Lk,
                         int32_t heads, int32_t d_k, float scale, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv,
                         int64_t lddv, ma_stream_t stream);

/* LabelSmoothingLoss (loss/label_smoothing_loss.py:24-117) on logits (rows, ld >= V) float32: stats[0] = sum over
 * unmasked rows of KL(true_dist || softmax), stats[1] = correct argmax count, stats[2] = unmasked rows (stored, round 4: no fill in
 * front of the call; the loss is stats[0] / batch, the accuracy stats[1] / stats[2], asr_model.py:188-209); the per-row terms go through
 * `row_stats` (rows x 3 floats of scratch) and are added in row order - no float atomics.
 * dlogits (rows, ld_out) bf16 (_f32) or float32 (_x32: the float32 validation mode) = grad_scale * mask * (softmax - true_dist),
 * zero in columns >= V.  `denom` (optional DEVICE float): `normalize_length=True` (label_smoothing_loss.py:106: the divisor is
 * the number of unmasked tokens instead of the batch size) - dlogits is divided by *denom (the caller's sum of the mask, no host
 * round trip) and the loss is stats[0] / stats[2]. */
int ma_label_smoothing_loss_grad_len_f32(const float* logits, int64_t ld, int64_t rows, int32_t V, const int32_t* target,
                                         const float* mask, float smoothing, float grad_scale, const float* denom, void* dlogits,
                                         int64_t ld_out, float* stats, float* row_stats, ma_stream_t stream);
int ma_label_smoothing_loss_grad_len_x32(const float* logits, int64_t ld, int64_t rows, int32_t V, const int32_t* target,
                                         const float* mask, float smoothing, float grad_scale, const float* denom, float* dlogits,
                                         int64_t ld_out, float* stats, float* row_stats, ma_stream_t stream);

/* ma_conv2d_3x3s2_nhwc_bf16 for the subsampling layer's second convolution (C = Cout = 256; layers/subsampling.py:40-45) on a
 * fragment-ordered packed copy of W (conv2_packed.hip): out (batch, Ho, Wo, 256) bf16 = [relu](bias + conv).
 *   ma_conv2d_3x3s2_packed_bytes(C, Cout) -> bytes of the packed buffer (negative: unsupported shape);
 *   ma_conv2d_3x3s2_pack_bf16(W (Cout, 3, 3, C) bf16, ..., packed): once per weight update. */
int64_t ma_conv2d_3x3s2_packed_bytes(int64_t C, int64_t Cout);
int ma_conv2d_3x3s2_pack_bf16(const void* W, int64_t C, int64_t Cout, void* packed, ma_stream_t stream);
int ma_conv2d_3x3s2_packed_nhwc_bf16(const void* act, int64_t batch, int64_t H, int64_t Wd, int64_t C, const void* packed,
                                     int64_t Cout, const float* bias, int32_t relu, void* out, ma_stream_t stream);

/* GlobalCMVN + BOTH convolutions of Conv2dSubsampling4 in one launch (subsample_fused.hip; layers/cmvn.py:33-35,
 * layers/subsampling.py:40-45): x (batch, T, idim) float32 with any element strides -> out (batch, T2, F2, C) bf16 NHWC =
 * relu(conv2(relu(conv1((x - mean) istd)))), T1 = (T - 3) / 2 + 1, T2 = (T1 - 3) / 2 + 1, same for the feature axis.  conv1's output
 * (what ma_subsample_conv1_strided_nhwc writes to memory) lives only in LDS, 32 channels at a time, and is computed on the matrix
 * pipe from bf16 head + tail splits of the float32 input and weight (x w = xh wh + xh wl + xl wh, relative error 2^-16 per
 * product before the rounding to bf16 that both paths apply).  Both weights come through one packed buffer:
 *   ma_subsample_fused_packed_bytes(idim, C) -> its size in bytes (negative: shape not covered - idim 80, C 256 only);
 *   ma_subsample_fused_pack_bf16(W1 (C, 9) float32, W2 (C, 3, 3, C) bf16, ..., packed): once per weight update.
 * b1, b2 (C) float32; cmvn_mean / cmvn_istd: both NULL or both (idim) float32. */
int64_t ma_subsample_fused_packed_bytes(int64_t idim, int64_t C);
int ma_subsample_fused_pack_bf16(const float* W1, const void* W2, int64_t idim, int64_t C, void* packed, ma_stream_t stream);
int ma_subsample_fused_bf16(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, int64_t batch, int64_t T,
                            int32_t idim, const float* cmvn_mean, const float* cmvn_istd, const void* packed, const float* b1,
                            const float* b2, int64_t C, void* out, ma_stream_t stream);
/* The same launch with its grid bounded.  ma_subsample_fused_bf16 runs a kernel whose workgroups WALK the 128-position tiles
 * (workgroup w takes tiles w, w + workgroups, ...; the next tile's input rows, im2col view and first patch are built under the
 * current tile's last chunk and epilogue) with one workgroup per compute unit; max_workgroups > 0 caps the grid instead (tests use
 * it for long walks on small inputs), 0 = that default, < 0 = MA_ERR_INVALID_ARG.  The output is bit-identical for every grid, and to
 * the one-tile-per-workgroup kernel, which MINDAUDIO_AMD_SUBSAMPLE=tile (read once per process) selects for
 * ma_subsample_fused_bf16. */
int ma_subsample_fused_walk_bf16(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, int64_t batch, int64_t T,
                                 int32_t idim, const float* cmvn_mean, const float* cmvn_istd, const void* packed, const float* b1,
                                 const float* b2, int64_t C, void* out, int32_t max_workgroups, ma_stream_t stream);

/* Input gradient of the same convolution without the im2col-shaped intermediate (conv2_dinput.hip; the training step's
 * replacement for ma_gemm (dy . W) + ma_col2im_3x3s2_relu_bf16): dact (batch, H, Wd, C) bf16 = [act > 0] * conv_transpose(dy, W),
 * dy (batch, Ho, Wo, C) bf16, wt = the TRANSPOSED weight ((kh, kw, c), co) bf16 row-major (row stride C), act (batch, H, Wd, C) bf16 or
 * NULL (no ReLU'), zero_row = at least 128 zero bytes in device memory (the source of taps outside the output grid).  C = Cout,
 * C % 128 == 0.  The float32 accumulator sums a position's taps (the two-launch form rounds each tap to bf16 first). */
int ma_conv2d_3x3s2_dinput_bf16(const void* dy, int64_t batch, int64_t H, int64_t Wd, int64_t C, const void* wt, const void* act,
                                const void* zero_row, void* dact, ma_stream_t stream);

/* Dense layer with a long contraction and 256 outputs on a fragment-ordered packed copy of W (rows_packed.hip): the `out`
 * Linear(19 * 256 -> 256) of Conv2dSubsampling4 followed by x * sqrt(d) (layers/subsampling.py:46-47,76, layers/embedding.py:84):
 *   out (M, 256) float32 = alpha * (A (M, K) bf16 . W (256, K)^T + bias).
 *   ma_gemm_rows_packed_bytes(N, K) -> bytes of the packed buffer (negative: unsupported; N = 256, K % 64 == 0; K is zero-padded to a multiple of 192);
 *   ma_gemm_rows_pack_bf16(W (N, K) bf16, ldw, N, K, packed): once per weight update. */
int64_t ma_gemm_rows_packed_bytes(int64_t N, int64_t K);
int ma_gemm_rows_pack_bf16(const void* W, int64_t ldw, int64_t N, int64_t K, void* packed, ma_stream_t stream);
int ma_gemm_rows_packed_f32(const void* A, int64_t lda, int64_t M, int64_t K, const void* packed, int64_t N, const float* bias,
                            float alpha, float* out, int64_t ldo, ma_stream_t stream);

/* ma_convmodule_mid_bf16 + pointwise_conv2 + mask_pad + the block's residual in one launch (layers/convolution.py:100-127,
 * models/conformer.py:143; C = 256, odd kernel_size <= 15):
 *   x[m, :] += mask[m] * (swish(bn(depthwise(glu(y))))[m, :] . Wp2^T + pw2_bias)
 * y (batch*T, 512) bf16; pw2_packed = ma_gemm_k256_pack_bf16 of the (256, 256) pointwise_conv2 weight; mask (batch*T) or NULL;
 * x (batch*T, 256) float32 updated in place. */
int ma_convmid_pw2_bf16(const void* y, int64_t ldy, int64_t batch, int64_t T, int32_t C, const float* dw, int32_t kernel_size,
                        const float* bn_scale, const float* bn_shift, const void* pw2_packed, const float* pw2_bias,
                        const float* mask, float* x, int64_t ldx, ma_stream_t stream);

/* The whole ConvolutionModule behind its LayerNorm in one launch (layers/convolution.py:96-127 + models/conformer.py:143;
 * C = 256, odd kernel_size <= 15): pointwise_conv1 + GLU + depthwise + BatchNorm(affine) + Swish + pointwise_conv2 + mask_pad +
 * the block's residual:
 *   x[m, :] += mask[m] * (swish(bn(depthwise(glu(a . Wp1^T + pw1_bias))))[m, :] . Wp2^T + pw2_bias)
 * a (batch*T, 256) bf16 = norm_conv(x) * mask_pad; pw1_packed / pw2_packed = ma_gemm_k256_pack_bf16 of the (512, 256) /
 * (256, 256) pointwise weights; mask (batch*T) or NULL; x (batch*T, 256) float32 updated in place. */
int ma_convmodule_bf16(const void* a, int64_t lda, int64_t batch, int64_t T, int32_t C, const void* pw1_packed,
                       const float* pw1_bias, const float* dw, int32_t kernel_size, const float* bn_scale, const float* bn_shift,
                       const void* pw2_packed, const float* pw2_bias, const float* mask, float* x, int64_t ldx,
                       ma_stream_t stream);

/* ma_convmodule_bf16 with the attention output projection, its residual and norm_conv in front (layers/attention.py:56 linear_out,
 * models/conformer.py:135-141): per 32-frame tile
 *   x' = x + ctx . Wo^T + wo_bias;   a = LN(x'; ln_gamma, ln_beta) * mask;   x_out <- x' + mask * ConvModule(a)
 * ctx (batch*T, 256) bf16 attention context; wo_packed = ma_gemm_k256_pack_bf16 of the (256, 256) linear_out weight.  x is read
 * and x_out written once; x' and a never leave the CU (the halo frames of a tile recompute the projection - from the residual rows
 * of the neighbouring tiles, which is why x_out must not overlap x: MA_ERR_INVALID_ARG.  Until ABI 3 the update was in place and
 * correct only while every workgroup of the launch was resident at the same time). */
int ma_attn_out_convmodule_bf16(const void* ctx, int64_t ldc, const void* wo_packed, const float* wo_bias, const float* ln_gamma,
                                const float* ln_beta, float ln_eps, int64_t batch, int64_t T, int32_t C, const void* pw1_packed,
                                const float* pw1_bias, const float* dw, int32_t kernel_size, const float* bn_scale,
                                const float* bn_shift, const void* pw2_packed, const float* pw2_bias, const float* mask, const float* x,
                                float* x_out, int64_t ldx, ma_stream_t stream);

/* Dense / k=1 Conv1d with K = 256 inputs (linear_q/k/v/out: layers/attention.py:51-56; pointwise_conv1/2:
 * layers/convolution.py:52-78) on a fragment-ordered packed copy of W (gemm_k256.hip): same result as ma_gemm_bf16.
 *   ma_gemm_k256_packed_bytes(N, K) -> bytes of the packed buffer (negative: unsupported; K = 256, N % 256 == 0);
 *   ma_gemm_k256_pack_bf16(W (N, K) bf16 row stride ldw, ..., packed): once per weight update;
 *   ma_gemm_k256_packed_bf16: epilogue as ma_gemm_bf16 without col_scale / col_shift / act2, act in {0, 1 swish, 2 relu}. */
int64_t ma_gemm_k256_packed_bytes(int64_t N, int64_t K);
int ma_gemm_k256_pack_bf16(const void* W, int64_t ldw, int64_t N, int64_t K, void* packed, ma_stream_t stream);
int ma_gemm_k256_packed_bf16(const void* A, int64_t lda, const void* packed, void* out, int64_t ldo, int64_t M, int64_t N,
                             int64_t K, const ma_gemm_epilogue_t* epi, ma_stream_t stream);
/* The same for N = 256 with the LayerNorm that follows fused behind the epilogue (a workgroup owns whole rows):
 * ln_out (M, 256) bf16 = LayerNorm(out[m, :]; ln_gamma, ln_beta, ln_eps) * ln_row_scale[m] (ln_row_scale may be NULL) — the
 * attention output projection + residual, then `norm_conv` and the mask_pad multiply (models/conformer.py:133-141,
 * layers/convolution.py:97-98), in one launch. */
int ma_gemm_k256_packed_ln_bf16(const void* A, int64_t lda, const void* packed, void* out, int64_t ldo, int64_t M, int64_t N,
                                int64_t K, const ma_gemm_epilogue_t* epi, const float* ln_gamma, const float* ln_beta,
                                float ln_eps, const float* ln_row_scale, void* ln_out, int64_t ld_ln, ma_stream_t stream);

/* PositionwiseFeedForward + residual (+ the LayerNorms around it) in ONE kernel, "hidden-slice owner" form (ffn_packed.hip;
 * layers/positionwise_feed_forward.py:33-46 with Swish, models/conformer.py:109-112 / 147-156):
 *     x[m, :] += alpha * (swish(a[m, :] . W1^T + b1) . W2^T + b2)
 *   a (M, 256) bf16 = LayerNorm(x) (or computed by the kernel, see gamma0); b1 (hidden), b2 (256) float32; x (M, 256) float32
 *   updated in place; the (M, hidden) activation never reaches HBM.  W1 / W2 are taken in a fragment-ordered packed form that
 *   lets them stream L2 -> registers without an LDS stage.  Pack once per weight update:
 *   ma_ffn_packed_bytes(d_model, hidden) -> bytes of the packed buffer (negative: unsupported shape; d_model = 256,
 *                                           hidden % 256 == 0);
 *   ma_ffn_pack_weights_bf16(w1 (hidden, d_model) bf16, w2 (d_model, hidden) bf16, ..., packed).
 * ma_ffn_packed_bf16: ln_mode 0 = no LayerNorm (gamma/beta/ln_out ignored);
 *   ln_mode 1: x += alpha * FFN(a);  ln_out = LN(x; gamma1, beta1)                       (macaron FFN -> norm_mha)
 *   ln_mode 2: x <- LN(x + alpha * FFN(a); gamma1, beta1);  ln_out = LN(x; gamma2, beta2)
 *              (FFN -> norm_final -> the next block's norm_ff_macaron / after_norm, models/conformer.py:147-156, 253)
 *   ln_out (M, 256) bf16 or float32 with row stride ld_ln.  gamma0 / beta0 non-NULL:
 * the input is a = LayerNorm(x; gamma0, beta0, eps) computed while the tile is staged (models/conformer.py:147-148) and the `a`
 * operand is ignored (may be NULL). */
int64_t ma_ffn_packed_bytes(int32_t d_model, int32_t hidden);
int ma_ffn_pack_weights_bf16(const void* w1, const void* w2, int32_t d_model, int32_t hidden, void* packed,
                             ma_stream_t stream);
int ma_ffn_packed_bf16(const void* a, int64_t lda, const void* packed, const float* b1, const float* b2, float* x,
                       int64_t ldx, int64_t M, int32_t d_model, int32_t hidden, float alpha, int32_t ln_mode,
                       const float* gamma1, const float* beta1, const float* gamma2, const float* beta2, float eps,
                       void* ln_out, int64_t ld_ln, int32_t ln_out_bf16, const float* gamma0, const float* beta0,
                       ma_stream_t stream);

/* Two FFNs on the same 64-row tiles in one launch: the last FFN of Conformer block i and the macaron FFN of block i + 1
 * (models/conformer.py:147-156 of block i, :109-112 of block i + 1), with the three LayerNorms between and after them:
 *   x1 = x + alpha FFN_A(LN(x; gamma0, beta0));  x2 = LN(x1; gamma1, beta1);  x <- x2 + alpha FFN_B(LN(x2; gamma2, beta2));
 *   ln_out = bf16 LN(x; gamma3, beta3)
 * x2 and the second FFN's input stay in LDS: one read and one write of the residual stream instead of two each.
 * packed_a / packed_b from ma_ffn_pack_weights_bf16 (same d_model = 256 and hidden). */
int ma_ffn_packed_pair_bf16(const void* packed_a, const float* b1_a, const float* b2_a, const void* packed_b, const float* b1_b,
                            const float* b2_b, float* x, int64_t ldx, int64_t M, int32_t d_model, int32_t hidden, float alpha,
                            const float* gamma0, const float* beta0, const float* gamma1, const float* beta1,
                            const float* gamma2, const float* beta2, const float* gamma3, const float* beta3, float eps,
                            void* ln_out, int64_t ld_ln, ma_stream_t stream);

/* The dense layer that consumes the final LayerNorm of ma_ffn_packed_bf16 (ln_mode 1) / ma_ffn_packed_pair_bf16 — linear_q/k/v of
 * the attention that follows (layers/attention.py:51-53, models/conformer.py:117-119) — run by the same launch on the tile while
 * it is in LDS:  qkv_out[m, :] = bf16(LN_out[m, :] . Wq^T + qkv_bias)   (qkv_out (M, qkv_n) bf16; LN_out itself is not written).
 * gamma0 / beta0 of ma_ffn_packed_qkv_bf16 (optional, then a may be NULL): the FFN input is LayerNorm(x; gamma0, beta0), as in
 * ma_ffn_packed_bf16.
 *   ma_ffn_qkv_packed_bytes(N) -> bytes of the packed weight (negative: unsupported; K = 256, N % 256 == 0, N <= 1024);
 *   ma_ffn_qkv_pack_bf16(W (N, 256) bf16, ldw, N, packed): once per weight update. */
int64_t ma_ffn_qkv_packed_bytes(int64_t N);
int ma_ffn_qkv_pack_bf16(const void* W, int64_t ldw, int64_t N, void* packed, ma_stream_t stream);
int ma_ffn_packed_qkv_bf16(const void* a, int64_t lda, const void* packed, const float* b1, const float* b2, float* x, int64_t ldx,
                           int64_t M, int32_t d_model, int32_t hidden, float alpha, const float* gamma0, const float* beta0,
                           const float* gamma1, const float* beta1, float eps, const void* qkv_packed, const float* qkv_bias,
                           int64_t qkv_n, void* qkv_out, int64_t ld_qkv, ma_stream_t stream);
int ma_ffn_packed_pair_qkv_bf16(const void* packed_a, const float* b1_a, const float* b2_a, const void* packed_b,
                                const float* b1_b, const float* b2_b, float* x, int64_t ldx, int64_t M, int32_t d_model,
                                int32_t hidden, float alpha, const float* gamma0, const float* beta0, const float* gamma1,
                                const float* beta1, const float* gamma2, const float* beta2, const float* gamma3,
                                const float* beta3, float eps, const void* qkv_packed, const float* qkv_bias, int64_t qkv_n,
                                void* qkv_out, int64_t ld_qkv, ma_stream_t stream);

/* TrainOneStepWithLossScaleCell pieces (train_one_step.py:37-47): *flag |= 1 if any gradient is inf/nan; Adam
 * (MindSpore nn.Adam: p -= lr_t * m / (sqrt(v) + eps), lr_t = lr sqrt(1-b2^t)/(1-b1^t) from the host) on
 * grad * inv_scale, skipped on the device when *overflow != 0. */
int ma_grad_overflow_f32(const float* g, int64_t n, int32_t* flag, ma_stream_t stream);
int ma_adam_f32(float* param, const float* grad, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                float eps, float inv_scale, const int32_t* overflow, ma_stream_t stream);
/* ma_adam_f32 + ma_cast_f32_bf16 of the updated parameters in one launch (round 4): mirror_bf16 (n) receives the bf16 conversion
 * (round to nearest even, as ma_cast_f32_bf16) of every updated parameter; untouched, like the parameters, when *overflow != 0.
 * Same parameter bits as ma_adam_f32.  n % 4 == 0, 16-byte aligned float buffers: MA_ERR_UNSUPPORTED otherwise. */
int ma_adam_mirror_f32(float* param, const float* grad, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                       float eps, float inv_scale, const int32_t* overflow, void* mirror_bf16, ma_stream_t stream);

/* Res2NetBlock (ecapatdnn.py:66-114) in one launch: y_0 = x_0, y_i = BN(ReLU(conv_{k=3,dil}(x_i + y_{i-1}) + b_i)), i = 1..scale-1
 * (y_1 from x_1 alone), x_i = columns [i cc, (i+1) cc) of x.  x, y: (batch, T + 2 halo, >= scale * cc) bf16 with zero halo rows
 * (pointers at the first halo row of utterance 0); w (scale-1, cc, 3 cc) bf16 with K = tap * cc + c; bias / bn_scale / bn_shift
 * (scale-1, cc) float32.  cc in {64, 128}, scale 8, dil <= halo, T + 2 halo <= 384, ldx % 8 == ldy % 8 == 0 and 16-byte aligned x, y, w
 * (MA_ERR_UNSUPPORTED otherwise); a workgroup owns one utterance for the whole chain. */
int64_t ma_res2net_fused_lds_bytes(int32_t cc, int64_t tp, int32_t dil);
int ma_res2net_fused_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t batch, int64_t T, int32_t halo, int32_t cc,
                          int32_t scale, int32_t dil, const void* w, const float* bias, const float* bn_scale,
                          const float* bn_shift, ma_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * float32 validation mode of the training step ("x32"): compute_type = float32 is the reference's default
 * (mindaudio/models/conformer.py:61, examples/conformer/asr_model.py:307-310).  Every activation and every product stays
 * float32, so the forward / backward / optimizer chain can be held to the north-star tolerance (loss curve within 1e-4 of a
 * float32 restatement of the reference); plain FMA kernels sized for validation shapes.  Semantics and argument meaning of
 * each entry = its bf16 form above with `float*` activations.
 * ---------------------------------------------------------------------------------------------- */
/* out (M, N) = epilogue(A . B):  A[m][k] = A[m * a_row_stride + k * a_col_stride],  B[k][n] = B[n * b_n_stride + k * b_k_stride].
 * NT (Dense forward, W stored (N, K)): b_n_stride = ldw, b_k_stride = 1.   NN (dX = dY . W, W (K, N) row-major): b_n_stride = 1,
 * b_k_stride = ldw.   TN (dW = dY^T . X): a_row_stride = 1, a_col_stride = ld(dY), b_n_stride = 1, b_k_stride = ld(X).
 * Epilogue as ma_gemm_bf16 with act in {0 none, 1 swish, 2 relu}, no column affine, float32 output (accumulate into `out` by
 * passing it as the residual). */
int ma_gemm_x32(const float* A, int64_t a_row_stride, int64_t a_col_stride, const float* B, int64_t b_n_stride,
                int64_t b_k_stride, float* out, int64_t ldo, int64_t M, int64_t N, int64_t K, const ma_gemm_epilogue_t* epi,
                ma_stream_t stream);
/* out[c] (+)= sum over rows of A[r][c]  (bias gradients) */
int ma_colsum_x32(const float* A, int64_t lda, int64_t rows, int64_t cols, float* out, int32_t accumulate, ma_stream_t stream);
/* RelPositionMultiHeadedAttention (layers/attention.py:214-235), d_k = 64: qkv (B*T, >= 3*H*64) = [q | k | v] rows, pos (T, H*64),
 * mask (B, T) (0 = padded key: additive -10000) -> ctx (B*T, H*64), lse (B, H, T).  Backward: dqkv as qkv, dpos / dbias_u /
 * dbias_v accumulate; workspace from ma_relpos_attention_bwd_x32_workspace_bytes. */
int ma_relpos_attention_fwd_x32(const float* qkv, int64_t ld_qkv, const float* pos, int64_t ld_pos, const float* bias_u,
                                const float* bias_v, const float* mask, int64_t batch, int64_t T, int32_t heads, int32_t d_k,
                                float* ctx, int64_t ld_ctx, float* lse, ma_stream_t stream);
int64_t ma_relpos_attention_bwd_x32_workspace_bytes(int64_t batch, int64_t T, int32_t heads);
int ma_relpos_attention_bwd_x32(const float* qkv, int64_t ld_qkv, const float* pos, int64_t ld_pos, const float* bias_u,
                                const float* bias_v, const float* mask, const float* ctx, int64_t ld_ctx, const float* dctx,
                                int64_t ld_dctx, const float* lse, int64_t batch, int64_t T, int32_t heads, int32_t d_k,
                                float* dqkv, int64_t ld_dqkv, float* dpos, int64_t ld_dpos, float* dbias_u, float* dbias_v,
                                void* workspace, int64_t workspace_bytes, ma_stream_t stream);
/* ... with the (batch, T, T) per-(query, key) chunk mask instead of the (batch, T) padding mask */
int ma_relpos_attention_fwd_qmask_x32(const float* qkv, int64_t ld_qkv, const float* pos, int64_t ld_pos, const float* bias_u,
                                      const float* bias_v, const float* mask_qk, int64_t batch, int64_t T, int32_t heads,
                                      int32_t d_k, float* ctx, int64_t ld_ctx, float* lse, ma_stream_t stream);
int ma_relpos_attention_bwd_qmask_x32(const float* qkv, int64_t ld_qkv, const float* pos, int64_t ld_pos, const float* bias_u,
                                      const float* bias_v, const float* mask_qk, const float* ctx, int64_t ld_ctx,
                                      const float* dctx, int64_t ld_dctx, const float* lse, int64_t batch, int64_t T,
                                      int32_t heads, int32_t d_k, float* dqkv, int64_t ld_dqkv, float* dpos, int64_t ld_dpos,
                                      float* dbias_u, float* dbias_v, void* workspace, int64_t workspace_bytes,
                                      ma_stream_t stream);
/* Conv2dSubsampling4 (layers/subsampling.py:21-78): conv1 with any input strides -> NHWC float32; explicit im2col of the 3x3
 * stride-2 valid window, col (B*Ho*Wo, 9*C) with k = (kh, kw, c) (conv2 = ma_gemm_x32 on it); backward pieces. */
int ma_subsample_conv1_nhwc_x32(const float* x, int64_t stride_b, int64_t stride_t, int64_t stride_f, int64_t batch, int64_t T,
                                int32_t idim, const float* cmvn_mean, const float* cmvn_istd, const float* w, const float* bias,
                                int32_t C, float* out, ma_stream_t stream);
int ma_im2col_3x3s2_nhwc_x32(const float* act, int64_t batch, int64_t H, int64_t Wd, int64_t C, float* col, ma_stream_t stream);
int ma_col2im_3x3s2_relu_x32(const float* dcol, const float* act, int64_t batch, int64_t H, int64_t Wd, int64_t C,
                             float* dact, ma_stream_t stream);
int ma_relu_bwd_x32(float* dy, const float* y, int64_t n, ma_stream_t stream);
int ma_subsample_conv1_dw_x32(const float* dact, const float* x, int64_t batch, int64_t T, int32_t idim,
                              const float* cmvn_mean, const float* cmvn_istd, int32_t C, float* dw, float* db,
                              void* workspace, int64_t workspace_bytes, ma_stream_t stream);
/* element-wise pieces of the block (layers/swish.py, the dropouts of models/conformer.py:109-151, layers/convolution.py:83-129) */
int ma_act_dropout_fwd_x32(const float* u, float* h, int64_t n, int32_t act, float p, uint32_t seed, uint32_t salt,
                           ma_stream_t stream);
int ma_act_dropout_bwd_x32(const float* u, const float* dh, float* du, int64_t n, int32_t act, float p, uint32_t seed,
                           uint32_t salt, ma_stream_t stream);
int ma_dropout_bwd_x32(const float* g, int64_t ldg, float* dy, int64_t ldy, int64_t rows, int64_t cols, float alpha,
                       const float* row_scale, float p, uint32_t seed, uint32_t salt, ma_stream_t stream);
int ma_convmid_fwd_train_x32(const float* y, int64_t ldy, int64_t batch, int64_t T, int32_t C, const float* dw_w,
                             int32_t ks, const float* dw_b, float* z, float* sums, ma_stream_t stream);
int ma_bn_swish_fwd_x32(const float* z, const float* stats, const float* gamma, const float* beta, float* out,
                        int64_t rows, int32_t C, ma_stream_t stream);
int ma_bn_swish_bwd_x32(const float* dout, const float* z, const float* stats, const float* gamma, const float* beta,
                        float* dz, int64_t rows, int32_t C, float* dsum, float* d_gamma, float* d_beta, void* workspace,
                        int64_t workspace_bytes, ma_stream_t stream);
int ma_convmid_bwd_x32(const float* dz, const float* y, int64_t ldy, int64_t batch, int64_t T, int32_t C,
                       const float* dw_w, int32_t ks, float* dy, int64_t lddy, float* d_dw_w, float* d_dw_b,
                       void* workspace, int64_t workspace_bytes, ma_stream_t stream);
/* ma_ctc_loss_grad_f32 with float32 dlogits */
int ma_ctc_loss_grad_x32(const float* logits, int64_t ld, int64_t batch, int64_t T, int32_t V, const int32_t* ys,
                         int32_t Lmax, const int32_t* hlens, const int32_t* ylens, int32_t blank,
                         int32_t zero_infinity, float grad_scale, float* per_utt_loss, float* lse_workspace,
                         float* loss_out, float* dlogits, int64_t ld_out, void* workspace, int64_t workspace_bytes,
                         ma_stream_t stream);

/* ---- a Conformer block's launches from one C call (round 4) --------------------------------------------------------------------
 * A block table holds, per (direction, block), the list of C-ABI calls of this header that make up the training-mode forward
 * (models/conformer.py:109-156: macaron FFN -> MHSA -> convolution module -> FFN -> norm_final) or backward of ONE encoder block at
 * one batch shape: entry point, argument words, copies of the host structs behind pointer arguments.  The host side (the training
 * engine, utils/train_one_step.py:13-48 on the reference side) fills it once per batch shape while it walks the block call by call,
 * and from then on issues the block with ONE call; the entries' device buffers must stay allocated while the table lives.
 *   ma_block_table_entry_point(name): index of a replayable entry point (int-returning, `ma_stream_t stream` last, only scalars,
 *     device pointers and pointers to the host structs ma_train_epilogue_t / ma_gemm_epilogue_t / ma_tn_item_t / ma_tn_direct_item_t /
 *     ma_melbank_t); -2 for a launch that is not (host out-pointers, host pointer tables: a recorded block must not contain one),
 *     -1 for anything else (size queries, unknown names);  ma_block_table_entry_point_params(fn): its parameter count;  _seeds(fn): bit k set = parameter k
 *     is a dropout seed (`uint32_t seed*`).
 *   ma_block_table_add: words[k] = parameter k as 8 bytes - pointer or integer as is, float / double as the bits of a double, a host
 *     struct (or host array) as its byte offset in `blob` (-1 = NULL; blob_bytes % 8 == 0; the blob is copied), the stream and seed
 *     parameters as anything (they are replaced).
 *   ma_conformer_block_fwd_train / _bwd_train: issue the block's calls in the order they were added, on `stream`, every `seed*`
 *     parameter and every ma_train_epilogue_t.seed = `seed` (the step's dropout stream).  MA_ERR_INVALID_ARG for a block without
 *     entries; an entry's own error code otherwise (ma_block_table_failed_call = its index). */
typedef struct ma_block_table ma_block_table_t;
ma_block_table_t* ma_block_table_create(void);
void ma_block_table_destroy(ma_block_table_t* table);
int32_t ma_block_table_entry_point(const char* name);
int32_t ma_block_table_entry_point_params(int32_t fn);
uint64_t ma_block_table_entry_point_seeds(int32_t fn);
int ma_block_table_add(ma_block_table_t* table, int32_t backward, int32_t block, int32_t fn, const int64_t* words, int32_t n_words,
                       const void* blob, int64_t blob_bytes);
int32_t ma_block_table_calls(const ma_block_table_t* table, int32_t backward, int32_t block);
int32_t ma_block_table_failed_call(const ma_block_table_t* table);
/* reading an entry back: its entry point (-1: no such entry), word k, and its blob (copies min(bytes, size) bytes; returns the size) */
int32_t ma_block_table_call_entry_point(const ma_block_table_t* table, int32_t backward, int32_t block, int32_t call);
int64_t ma_block_table_call_word(const ma_block_table_t* table, int32_t backward, int32_t block, int32_t call, int32_t k);
int64_t ma_block_table_call_blob(const ma_block_table_t* table, int32_t backward, int32_t block, int32_t call, void* out, int64_t bytes);
int ma_conformer_block_fwd_train(ma_block_table_t* table, int32_t block, uint32_t seed, ma_stream_t stream);
int ma_conformer_block_bwd_train(ma_block_table_t* table, int32_t block, uint32_t seed, ma_stream_t stream);

/* ---- speaker verification scoring (examples/ECAPA-TDNN/speaker_verification_cosine.py: emb_mean, evaluate2) --------------------
 * Embedding width D: a multiple of 32 up to 512, anything else MA_ERR_INVALID_ARG.  All launches are asynchronous on `stream`, none
 * allocates, results are bit-identical from run to run (float64 sums in a fixed order, no floating-point atomics).
 *   ma_cohort_stats_f32: mean[e] / std[e] (float64) = np.mean / np.std of the K largest cos(Q[e], C[n]) over n - the multiset
 *     np.partition(s, kth=-K)[-K:] holds (K == N: all of them; K > N or K < 1: MA_ERR_INVALID_ARG).  Q (E, D), C (N, D) raw float32
 *     rows, 16-byte aligned, ld % 4 == 0; a zero-norm row scores 0 against everything.  Scores are the exact-float32 MFMA product
 *     scaled by float64 inverse norms and rounded to float32 once; the selection is an exact radix select on those float32 scores.
 *     The workspace holds the norms and the score block of as many query rows as fit (at least one row: MA_ERR_WORKSPACE otherwise);
 *     ma_cohort_stats_workspace_bytes(E, N) is the size for blocks of 512 rows.
 *   ma_trial_scores_f32: score[t] (float64) = cos(emb[enrol_idx[t]], emb[test_idx[t]]), normalised with the per-embedding mean / std
 *     of ma_cohort_stats_f32: MA_SCORE_NORM_Z (s - mean_e) / std_e, _T (s - mean_t) / std_t, _S the half-sum of the two, _NONE as is
 *     (mean / std may then be NULL).  An index outside [0, n_emb) gives NaN.
 *   ma_running_mean_sub_f32: Y[n] = X[n] - g_n, g_n = (1 - w) g_{n-1} + w X[n], w = 1 / (count + n + 1) (g_0 = X[0] when count == 0),
 *     evaluated as the cumulative mean in float64; g_mean (D float64, device) is read as g_{-1} and left as g_{N-1}; the caller's
 *     new count is count + N.  Y may alias X.
 *   ma_sentence_mean_norm_f32: out[b, t, f] = x[b, t, f] - mean_t x[b, t, f]  (InputNormalization "sentence", std_norm=False). */
#define MA_SCORE_NORM_NONE 0
#define MA_SCORE_NORM_Z 1
#define MA_SCORE_NORM_T 2
#define MA_SCORE_NORM_S 3
int64_t ma_cohort_stats_workspace_bytes(int64_t E, int64_t N);
int ma_cohort_stats_f32(const float* Q, int64_t ldq, const float* C, int64_t ldc, int64_t E, int64_t N, int32_t D, int64_t K,
                        double* mean, double* stdev, void* workspace, int64_t workspace_bytes, ma_stream_t stream);
int ma_trial_scores_f32(const float* emb, int64_t ld, int64_t n_emb, int32_t D, const int32_t* enrol_idx, const int32_t* test_idx,
                        int64_t T, const double* mean, const double* stdev, int32_t mode, double* score, ma_stream_t stream);
int64_t ma_running_mean_sub_workspace_bytes(int64_t N, int32_t D);
int ma_running_mean_sub_f32(const float* X, int64_t ldx, int64_t N, int32_t D, double* g_mean, int64_t count, float* Y, int64_t ldy,
                            void* workspace, int64_t workspace_bytes, ma_stream_t stream);
int ma_sentence_mean_norm_f32(const float* x, int64_t batch, int64_t T, int32_t F, float* out, ma_stream_t stream);

/* ---- waveform augmentation chain (csrc/augment.hip; mindaudio.data.augment, examples/ECAPA-TDNN/spec_augment.py) ----------------
 * Rows are float32 waveforms `x + r * ldx` of n samples; every entry point that writes waveforms takes (out, ldo, n_out) and writes
 * n_out columns per row: the result for columns < n (cut when n_out < n), 0.0 for columns in [n, n_out) - so an augmenter can
 * write straight into its slice of the matrix the fbank reads.  Nothing allocates, nothing reads a scalar back: amplitudes live in
 * a statistics buffer `double stats[rows][4]` = { sum |x|, sum x^2, max |x|, 0 } that the next kernel reads.  All sums run in a fixed
 * order (no atomics): results are bit-identical from run to run.  rows <= 65535.
 *   row_stats: the statistics of every row over its first n samples, float64 accumulation, one launch.
 *   circular_fir: y[r][i] = sum_{k<K} h[k] x[r][(i - k) mod n], one filter (device, K <= 255 taps) for the batch; out must not
 *     alias x.  (drop_freq: the reference's un-centred circular convolution.)
 *   fft_conv: y[r][i] = sum_{k<K} h[k] x[r][(i + rot - k) mod n] (convolve1d(use_fft=True, rotation_index=rot); K <= n,
 *     0 <= rot <= K) through zero-padded transforms of length L = ma_aug_fft_conv_length(n, K) (power of two >= n + K - 1), two rows
 *     per complex transform, the filter's spectrum once per call; the wrapped tail is folded back in the pass that writes y.
 *     stats_x != NULL: y is then rescaled to the input's average amplitude, y * amp(x) / (amp(y) + 1e-14), amp = sum|.| / n
 *     (reverberate, rescale_amp="avg").  out may alias x.
 *   babble_sum: out[r] = x[r - 1] + x[r - 2] + ... + x[r - speakers] (row indices mod rows, added in that order).
 *   mix: out[r][i] = a_r x[r][i] + s_r noise[r * ld_noise + i] (ld_noise == 0: one noise row for the batch); out may alias x.
 *     MA_AUG_MIX_NOISE   a = 1, s = gain * sqrt(stats_x[r].sumsq / n)                               (add_noise; gain = 10^(-snr/20))
 *     MA_AUG_MIX_BABBLE  a = 1 - f, s = f * (sx / len) / (sn / blen + 1e-14), params[r] = { f, len, blen, 0 } (double)  (add_babble)
 *     MA_AUG_MIX_UNIT_AVG  a = gain / (sx / len + 1e-14), params[r] = { len, .. }; MA_AUG_MIX_UNIT_PEAK  a = gain / (max|x| + 1e-14);
 *       MA_AUG_MIX_UNIT_RMS  a = gain / (sqrt(sx2 / n) + 1e-8); all three with s = 0 and noise unused (unitarize / rescale /
 *       rms_normalize).
 *   drop_chunks: out = x with the intervals [start, end) of `intervals` (int32 (rows, n_max, 2), clipped to [0, n), empty ones
 *     allowed, n_max <= 256) replaced in order j = 0 .. n_max - 1 (a later interval wins): by 0.0 when fill == NULL, else by
 *     2 m u - m, m = 2 noise_factor stats[r].sumabs / lens[r], u = fill[fill_off[r * n_max + j] + i - start] (the host's uniform
 *     draws, one run per interval).  Samples outside every interval are copied bit for bit.  out must not alias x. */
#define MA_AUG_MIX_NOISE 0
#define MA_AUG_MIX_BABBLE 1
#define MA_AUG_MIX_UNIT_AVG 2
#define MA_AUG_MIX_UNIT_PEAK 3
#define MA_AUG_MIX_UNIT_RMS 4
int ma_aug_row_stats_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, double* stats, ma_stream_t stream);
int ma_aug_circular_fir_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, const float* h, int32_t K, float* out,
                            int64_t ldo, int64_t n_out, ma_stream_t stream);
int64_t ma_aug_fft_conv_length(int64_t n, int64_t K);
int64_t ma_aug_fft_conv_workspace_bytes(int64_t rows, int64_t n, int64_t K);
int ma_aug_fft_conv_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, const float* h, int64_t K, int64_t rot,
                        const double* stats_x, float* out, int64_t ldo, int64_t n_out, void* workspace, int64_t workspace_bytes,
                        ma_stream_t stream);
int ma_aug_babble_sum_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, int32_t speakers, float* out, int64_t ldo,
                          ma_stream_t stream);
int ma_aug_mix_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, const float* noise, int64_t ld_noise, int32_t mode,
                   float gain, const double* params, const double* stats_x, const double* stats_noise, float* out, int64_t ldo,
                   int64_t n_out, ma_stream_t stream);
int ma_aug_drop_chunks_f32(const float* x, int64_t ldx, int64_t rows, int64_t n, const int32_t* intervals, int32_t n_max,
                           const float* fill, const int32_t* fill_off, float noise_factor, const double* stats, const double* lens,
                           float* out, int64_t ldo, int64_t n_out, ma_stream_t stream);

/* ---- ECAPA speaker-classification head (mindaudio/models/ecapatdnn.py:477-488 Classifier.construct with lin_blocks = 0,
 * mindaudio/loss/AdditiveAngularMargin.py:27-39, and SoftmaxCrossEntropyWithLogits(sparse=False, reduction="mean") / CorrectLabelNum
 * of examples/ECAPA-TDNN/train_speaker_embeddings.py:273-317) ------------------------------------------------------------------
 * x (B, D) embeddings, W (N, D) class weights, y (B) int32 labels; contiguous float32, 16-byte aligned.  D a multiple of 32 in
 * [32, 512] (anything else MA_ERR_UNSUPPORTED), B >= 1, N >= 2.  float32 operands and accumulation (f32 MFMA), accurate exp / log,
 * no floating-point atomics: two runs give the same bits.  All launches are asynchronous on `stream`, none allocates.
 *   e_i = x_i / sqrt(max(sum x_i^2, eps)), w_j likewise (MindSpore's L2Normalize); c = e w^T; sine = sqrt(max(1 - c^2, 0));
 *   phi = c cos m - sine sin m, kept where c > cos(pi - m) (easy_margin: c > 0), else c - sin(pi - m) m (easy_margin: c);
 *   output = scale (onehot phi + (1 - onehot) c); row_loss_i = logsumexp_j output_ij - output_i,y_i; loss = mean_i row_loss_i;
 *   correct = sum_i [argmax_j output_ij == y_i], ties to the lowest index.
 *   A label outside [0, N) is never used as an index: that row has no target (row_loss = its logsumexp, never correct).
 *   ma_aam_softmax_fwd_f32 (3 launches): output (B, N), row_loss (B), loss (1), correct (1), and what the backward reads again:
 *     inv_x (B), inv_w (N) the inverse norms, lse (B) the log-sum-exp, tgrad (B) d phi / d c of the target column
 *     (cos m + sin m c / max(sine, 2^-12) on the phi branch, 1 on the other; rows without a target are left unwritten).
 *   ma_aam_softmax_bwd_f32 (3 launches): dx (B, D) and dW (N, D) = *grad_scale times the exact derivative of `loss`, both
 *     normalisations included (a row with sum r^2 <= eps is divided by the constant sqrt(eps), and differentiated as that);
 *     dW additionally receives l2 * W.  grad_scale is a device scalar.  Probabilities are recomputed from `output` and `lse`.
 *   Workspace: ma_aam_softmax_workspace_bytes(B, D, N) serves either call (forward: three (B, ceil(N / 32)) partial arrays; backward:
 *     (S, B, D) partial sums of dx over S <= 64 slabs of classes); 16-byte aligned, MA_ERR_WORKSPACE when too small.
 *   ma_aam_cosine_f32 (2 launches): cosine (B, N) = c alone, with the inverse norms (Classifier.construct).
 *   ma_aam_margin_f32: out[i] = scale (targets[i] phi(cosine[i]) + (1 - targets[i]) cosine[i]) on n elements
 *     (AdditiveAngularMargin.construct on given cosines and one-hot targets). */
int64_t ma_aam_softmax_workspace_bytes(int64_t B, int32_t D, int64_t N);
int ma_aam_softmax_fwd_f32(const float* x, const float* W, const int32_t* y, int64_t B, int32_t D, int64_t N, float margin, float scale,
                           int32_t easy_margin, float eps, float* output, float* row_loss, float* loss, int32_t* correct, float* inv_x,
                           float* inv_w, float* lse, float* tgrad, void* workspace, int64_t workspace_bytes, ma_stream_t stream);
int ma_aam_softmax_bwd_f32(const float* x, const float* W, const int32_t* y, int64_t B, int32_t D, int64_t N, float scale, float eps,
                           const float* output, const float* inv_x, const float* inv_w, const float* lse, const float* tgrad,
                           const float* grad_scale, float l2, float* dx, float* dW, void* workspace, int64_t workspace_bytes,
                           ma_stream_t stream);
int ma_aam_cosine_f32(const float* x, const float* W, int64_t B, int32_t D, int64_t N, float eps, float* cosine, float* inv_x,
                      float* inv_w, ma_stream_t stream);
int ma_aam_margin_f32(const float* cosine, const float* targets, int64_t n, float margin, float scale, int32_t easy_margin, float* out,
                      ma_stream_t stream);

/* ---- phase vocoder (mindaudio/data/augment.py:828-871 _phase_vocoder; time_stretch :795-825 and pitch_shift :874-901 are
 * ma_stft_f32 -> this -> ma_istft_f32 (-> ma_resample_fft_f32), with no layout copy in between) -----------------------------------
 * spec: complex64 as interleaved float32, (B, frames, n_freq) for in_layout MA_STFT_FRAME_MAJOR (what ma_stft_f32 writes) or
 * (B, n_freq, frames) for MA_STFT_FREQ_MAJOR.  out: complex64 (B, n_freq, T_out), what ma_istft_f32 reads.  step_index (int32) and
 * step_alpha (float64), T_out device entries each: the integer and fractional parts of np.arange(0, frames, rate).
 * Step t, i = step_index[t], a = step_alpha[t], c_j = column j of the row (zero for j outside [0, frames), never read there - the
 * reference pads two zero columns):
 *   out[t] = ((1 - a) |c_i| + a |c_i+1|) (cos acc_t, sin acc_t),   acc_0 = angle(c_0),
 *   acc_t+1 = acc_t + phi + wrap(angle(c_i+1) - angle(c_i) - phi),  wrap(d) = d - 2 pi round(d / 2 pi),
 *   phi[k] = np.linspace(0, pi hop, n_freq)[k].
 * Angles, magnitudes, the mix, sine and cosine are float32.  phi, wrap and acc are float64, acc is reduced modulo 2 pi in float64
 * before the sine and cosine; the reference keeps acc in the spectrogram's precision (float32 for complex64) and loses what that
 * costs.  acc is a chunked scan over t with a summation order that depends on T_out only, without atomics: results are bit-identical
 * from run to run and for a row computed alone or inside a batch.
 * MA_ERR_HOP for hop < 1; MA_ERR_INVALID_ARG for B, frames or T_out < 1, n_freq < 2, an unknown layout or a null pointer. */
int ma_phase_vocoder_f32(const float* spec, int32_t in_layout, int64_t B, int64_t frames, int32_t n_freq, const int32_t* step_index,
                         const double* step_alpha, int64_t T_out, int32_t hop, float* out, ma_stream_t stream);

/* ---- IIR filters (mindaudio/data/filters.py: cal_filter_by_coffs :79-122 behind low_pass_filter and peaking_equalizer; filtfilt
 * :342-370 = scipy.signal.butter + scipy.signal.filtfilt) --------------------------------------------------------------------------
 * x, y: (rows, T) contiguous device samples, float32 (sample_bytes 4) or float64 (sample_bytes 8); y may be x.  Every row is
 * filtered by the order-n recursion in the transposed direct form II of scipy.signal.lfilter, n = filter->order, 1 <= n <= 16:
 *   y[t] = b[0] x[t] + z_0,   z_i = b[i+1] x[t] + z_(i+1) - a[i+1] y[t]  (i < n, z_n = 0).
 * Coefficients, state and arithmetic are float64 (fused multiply-adds); a sample is converted on the way in and rounded on the way
 * out.  ma_iir_filter_t lives in HOST memory, and so do the arrays it points to (they travel as kernel arguments):
 *   b, a     n + 1 coefficients each, normalised: a[0] == 1
 *   zi       n initial state values or NULL (zero state); zi_mode says how they are used: MA_IIR_ZI_NONE (ignored), MA_IIR_ZI_AS_IS,
 *            MA_IIR_ZI_TIMES_X0 (zi * the row's first sample in processing order: what scipy.signal.filtfilt does)
 *   reverse  != 0: the row is walked from its last sample to its first and every result is written where its sample was read
 *            (filtfilt's backward pass without flipped copies)
 *   upper_clamp  != 0: min(y[t], 1.0) is what is stored; the recursion goes on from the unclamped y[t] (cal_filter_by_coffs)
 *   chunk    L >= 1.  A row is cut into C = ceil(T / min(L, T)) chunks, one thread each: every chunk but the last runs from a zero
 *            state, the final states s_c are carried in order, z_(c+1) = P z_c + s_c, and every chunk runs again from its true state.
 *   power    P = A^L, n x n row-major, A[i][0] = -a[i+1], A[i][i+1] = 1: needed (and read) only when C > 1.  The caller decides
 *            whether P is usable - poles strictly inside the unit circle and P finite; otherwise it passes chunk >= T and every row
 *            is one sequential recursion (mindaudio_amd.data.filters.iir_plan).
 *   steps    0: everything.  Otherwise a mask of MA_IIR_STEP_* - only those of the three launches run, for timing them one by one
 *            (tools/iir_filter_bench.py); y or the workspace is then incomplete.  With C == 1 there is only MA_IIR_STEP_EMIT.
 * workspace: ma_iir_filter_workspace_bytes(rows, T, n, chunk) bytes of device memory, 8-byte aligned (0 bytes when C == 1).
 * No atomics; the order of every sum depends on T, L and n only: bit-identical from run to run and for a row alone or in a batch.
 * MA_ERR_INVALID_ARG for a null x, y, filter, b or a, a null power when C > 1, rows, T, n or chunk < 1, a[0] != 1, an unknown
 * zi_mode, steps or sample_bytes; MA_ERR_UNSUPPORTED for n > 16 or T >= 2^31 - 256; MA_ERR_WORKSPACE.  Nothing is launched on a refusal. */
#define MA_IIR_MAX_ORDER 16
#define MA_IIR_ZI_NONE 0
#define MA_IIR_ZI_AS_IS 1
#define MA_IIR_ZI_TIMES_X0 2
#define MA_IIR_STEP_CHUNK_STATES 1
#define MA_IIR_STEP_CARRY 2
#define MA_IIR_STEP_EMIT 4
typedef struct ma_iir_filter {
  int32_t order;
  int32_t zi_mode;
  int32_t reverse;
  int32_t upper_clamp;
  int64_t chunk;
  const double* b;
  const double* a;
  const double* zi;
  const double* power;
  int32_t steps;
  int32_t reserved;
} ma_iir_filter_t;
int64_t ma_iir_filter_workspace_bytes(int64_t rows, int64_t T, int32_t order, int64_t chunk);
int ma_iir_filter(const void* x, int32_t sample_bytes, int64_t rows, int64_t T, const ma_iir_filter_t* filter, void* y, void* workspace,
                  int64_t workspace_bytes, ma_stream_t stream);

/* ---- silence front end and reductions of mindaudio/data/processing.py (trim :263-319, split :322-377, normalize :28-95,
 * stereo_to_mono :235-260) -------------------------------------------------------------------------------------------------------------
 * Frames.  A row of n samples is zero-padded by frame_length / 2 on both sides and has
 *   F(n) = (n + 2 (frame_length / 2) - frame_length) / hop_length + 1
 * frames, which is n / hop_length + 1 for an even frame_length and (n - 1) / hop_length + 1 for an odd one (the reference's frame()
 * on the padded signal); frame f covers the padded positions [f hop_length, f hop_length + frame_length).
 * ma_frame_power_frames: F(n) on the host, MA_ERR_INVALID_ARG for n, frame_length or hop_length < 1.
 *
 * ma_frame_power: x (B, T) float32 (sample_bytes 4) or float64 (8), row stride ldx >= T; lengths: B int32 on the device (clamped to
 * [0, T]; a row of length 0 has no frames) or NULL (every row has T samples).  power (B, ldp) float64, ldp >= F(T):
 *   power[b][f] = sqrt(mean(x^2))^2 for f < F(lengths[b]) - the mean in float64, then the reference's square root and square -
 *   and 0 behind it; row_max[b] = the largest of them (0 for a row without frames).
 * Where hop_length divides frame_length and the ratio is at most MA_FRAME_POWER_MAX_RATIO a frame is the sum, in index order, of its
 * hop blocks' sums; otherwise a frame is summed directly.  A workgroup owns MA_FRAME_POWER_TILE frames.  No atomics, the order of
 * every sum depends on frame_length and hop_length only: bit-identical from run to run and for a row alone or inside a batch.
 *
 * ma_silence_edges: power as above; ref_rows: B float64 reference values on the device (ma_frame_power's row_max) or NULL, then
 * ref_scalar for every row.  In float64,
 *   nonsilent[b][f] = 10 log10(max(power, 1e-10)) - 10 log10(max(1e-10, ref)) > -top_db   for f < F(lengths[b]), 0 behind it
 * (nonsilent (B, ldp) uint8).  A boundary is an index i in [0, F] at which the flag changes, both ends counting as silent.
 *   trim_index (B, 2) int32: first boundary * hop_length, last boundary * hop_length (NOT clipped to the length, as trim leaves it)
 *   counts (B,) int32: intervals = boundaries / 2;  edges (B, ldp + 1) int32: min(boundary * hop_length, limit) in order, i.e.
 *   (start, end) pairs, -1 behind them; limit = clip when clip >= 0, else the row's length (split clips with shape[-1]).
 * A row without a non-silent frame has count 0 and trim_index (-1, -1).
 *
 * ma_axis_stats: x viewed as (outer, n, inner) contiguous, dtype MA_DTYPE_*; out (outer, inner) float64 = the statistic MA_AXIS_*
 * of |x| over n, in float64: maximum, minimum (a NaN wins both), count of |x| > 0, sum, sum of squares, mean = sum / n, and the
 * population standard deviation sqrt(sum (|x| - mean)^2 / n).  n is cut into 256 / min(64, pow2 >= inner) slices summed in index
 * order and joined by a halving tree: the order depends on n and inner only.
 *
 * ma_axis_apply: out = (x - sub) / div element by element in float64, sub and div (outer, inner) float64 statistics broadcast
 * over n, either of them NULL (left out; both NULL: MA_ERR_INVALID_ARG).  out has x's dtype (out_dtype == dtype: the float64
 * result is rounded to float32, or truncated toward zero to an integer, as an assignment into np.empty_like does) or is float64
 * (out_dtype == MA_DTYPE_F64).  out must not be x.
 *
 * ma_channel_mean: x (n, channels) channel last, float32 or float64 -> out (n,) of the same type: the channels added in that type
 * in the order of NumPy's add.reduce - index order below 8 channels, ((0+1)+(2+3))+((4+5)+(6+7)) at 8 - then divided by the
 * channel count, so that the result equals np.mean(x, axis=-1) bit for bit.  channels > MA_CHANNEL_MEAN_MAX: MA_ERR_UNSUPPORTED.
 *
 * All five: MA_ERR_INVALID_ARG for a null pointer, B, T, n, outer, inner, channels, frame_length or hop_length < 1, ldx < T,
 * ldp < F(T), an unknown sample_bytes, dtype or stat; MA_ERR_UNSUPPORTED where a position would not fit int32.  Nothing is launched
 * on a refusal. */
#define MA_FRAME_POWER_TILE 16
#define MA_FRAME_POWER_MAX_RATIO 32
#define MA_CHANNEL_MEAN_MAX 8
#define MA_DTYPE_F32 0
#define MA_DTYPE_F64 1
#define MA_DTYPE_I32 2
#define MA_DTYPE_I64 3
#define MA_AXIS_MAX 0
#define MA_AXIS_MIN 1
#define MA_AXIS_L0 2
#define MA_AXIS_SUM 3
#define MA_AXIS_SUMSQ 4
#define MA_AXIS_MEAN 5
#define MA_AXIS_STD 6
int64_t ma_frame_power_frames(int64_t n, int32_t frame_length, int32_t hop_length);
int ma_frame_power(const void* x, int32_t sample_bytes, int64_t B, int64_t T, int64_t ldx, const int32_t* lengths,
                   int32_t frame_length, int32_t hop_length, double* power, int64_t ldp, double* row_max, ma_stream_t stream);
int ma_silence_edges(const double* power, int64_t ldp, int64_t B, int64_t T, const int32_t* lengths, int32_t frame_length,
                     int32_t hop_length, const double* ref_rows, double ref_scalar, double top_db, int64_t clip, uint8_t* nonsilent,
                     int32_t* trim_index, int32_t* counts, int32_t* edges, ma_stream_t stream);
int ma_axis_stats(const void* x, int32_t dtype, int64_t outer, int64_t n, int64_t inner, int32_t stat, double* out,
                  ma_stream_t stream);
int ma_axis_apply(const void* x, int32_t dtype, int64_t outer, int64_t n, int64_t inner, const double* sub, const double* div, void* out,
                  int32_t out_dtype, ma_stream_t stream);
int ma_channel_mean(const void* x, int32_t sample_bytes, int64_t n, int32_t channels, void* out, ma_stream_t stream);

/* ---- harmonic / percussive separation of mindaudio/data/features.py (soft_mask :438-469, hpss :472-529) ---------------------------
 * ma_median_filter: a 1-D median filter of k taps along the axis n of a strided view (rows, n, inner), dtype MA_DTYPE_F32 or
 * MA_DTYPE_F64; x_strides and out_strides are three ELEMENT strides each (rows, n, inner), so one entry serves the time axis and
 * the frequency axis of a (B, F, T) spectrogram in either memory order, without a copy.  The semantics are those of
 * scipy.ndimage.median_filter(size=k, mode="reflect", origin=0) along that axis:
 *   the window of output i covers the indices i - k / 2 ... i - k / 2 + k - 1 (an even k leans left);
 *   the result is the element of rank k / 2 of the sorted window (an even k takes the upper middle, nothing is averaged);
 *   an index j outside [0, n) is read at j mod 2n, and at 2n - 1 - that where it is >= n: d c b a | a b c d | d c b a.
 * SciPy leaves this periodic reflection once the window is about 8n wide, so 1 <= k <= MA_MEDIAN_MAX_K and k <= 4n are required
 * (MA_ERR_INVALID_ARG otherwise).  The output is one of the window's inputs, bit for bit: element j wins when
 *   #(w[m] < w[j]) + #(w[m] == w[j], m < j) == k / 2,
 * which exactly one j does whatever the ties (where the tied values are +0 and -0, which of the two zeros comes out is not
 * specified).  Inputs are finite: the result for a window that holds a NaN is not specified.  A workgroup stages
 * MA_MEDIAN_SEGMENT outputs' worth of a few lines, plus the k - 1 halo with the reflection applied, in LDS.  No atomics: the same bits
 * from run to run and for a row alone or inside a batch.  out must not overlap x.
 *
 * ma_soft_mask: count elements, a, b (and spec, mask, out) of dtype MA_DTYPE_F32 or MA_DTYPE_F64 laid out alike.  With
 * x = a * (T)scale_a and r = b * (T)scale_b in the arrays' type T, the reference's order of operations, each correctly rounded
 * and none contracted into an FMA:
 *   z = max(x, r); bad = z < tiny(T) (FLT_MIN / DBL_MIN); z = 1 where bad; m = (x / z) ** power, rm = (r / z) ** power;
 *   m = m / (m + rm), and where bad 0, or 0.5 if split_zeros.
 * ** 1 is the value itself, ** 2 the product v * v, ** 0.5 the square root (NumPy's fast paths); every other power is powf / pow
 * with (T)power.  power = +inf: m = x > r.  power <= 0 or NaN: MA_ERR_INVALID_ARG.
 *   mask (optional): m as T, or for power = +inf as uint8 0 / 1.
 *   out (optional, with spec): spec * m as T; with phase (count complex64 pairs, float32 only) the complex64 (spec * m) * phase.
 *   negative (optional): one int32 on the device, set to 1 (a plain store; never cleared here) when any x or r is < 0.
 * At least one of mask and out is given.
 *
 * Both: MA_ERR_INVALID_ARG for a null pointer, a dimension < 1 or an unknown dtype, MA_ERR_UNSUPPORTED where the grid would not fit
 * 31 bits.  Nothing is launched on a refusal.
 *
 * ma_stft_frames_c32: the frames of ma_stft_f32 before the transform, for the n_fft its fused kernels do not cover (spectrum.stft
 * sends a power-of-two n_fft above 1024 - harmonic's 2048 - through ma_fft_pow2_c32): x (batch, n) float32 with row stride ldx,
 * frames (batch, n_frames, n_fft) complex64 as float pairs = (window[i] * padded x[f * hop - pad + i], 0), pad = n_fft / 2 when
 * center else 0, the padding np.pad's MA_PAD_* mode; n_frames must be ma_num_frames(n, n_fft, hop, center).  The errors of
 * ma_stft_f32; batch > 65535: MA_ERR_UNSUPPORTED.
 *
 * ma_istft_rows_c32 / ma_istft_ola_c32: the way back for the same n_fft, around the inverse ma_fft_pow2_c32.  ma_istft_f32 adds a
 * frame's n_fft / 2 terms one after the other in float32; at n_fft = 2048 that rounding is several times everything else in
 * features.harmonic.  ma_istft_rows_c32: spec (batch, n_fft / 2 + 1, frames_total) complex64 bin-major -> rows (batch, n_frames,
 * n_fft) complex64, the Hermitian extension of each of the first n_frames frames (imaginary parts of the DC and Nyquist bins
 * dropped).  ma_istft_ola_c32: rows = their unnormalised inverse transforms -> out (batch, out_len), ma_istft_f32's synthesis
 * window, overlap-add, division by the window sum-square (> 1e-9) and `start` offset, on real(rows) / n_fft.  The errors of
 * ma_istft_f32. */
#define MA_MEDIAN_MAX_K 127
#define MA_MEDIAN_SEGMENT 64
int ma_median_filter(const void* x, int32_t dtype, int64_t rows, int64_t n, int64_t inner, int64_t x_stride_rows, int64_t x_stride_n,
                     int64_t x_stride_inner, int32_t k, void* out, int64_t out_stride_rows, int64_t out_stride_n,
                     int64_t out_stride_inner, ma_stream_t stream);
int ma_soft_mask(const void* a, const void* b, int32_t dtype, int64_t count, double scale_a, double scale_b, double power,
                 int32_t split_zeros, void* mask, const void* spec, const void* phase, void* out, int32_t* negative,
                 ma_stream_t stream);
int ma_stft_frames_c32(const float* x, int64_t batch, int64_t n, int64_t ldx, int32_t n_fft, int32_t hop, const float* window,
                       int32_t center, int32_t pad_mode, float* frames, int64_t n_frames, ma_stream_t stream);
int ma_istft_rows_c32(const float* spec, int64_t batch, int32_t n_fft, int64_t frames_total, int64_t n_frames, float* rows,
                      ma_stream_t stream);
int ma_istft_ola_c32(const float* rows, int64_t batch, int32_t n_fft, int64_t n_frames, int32_t hop, const float* window,
                     int32_t start, float* out, int64_t out_len, ma_stream_t stream);

/* ---- Conv-TasNet separation (mindaudio/models/conv_tasnet.py, mindaudio/loss/separation_loss.py) -------------------------------------
 * The 1 x 1 convolutions are ma_gemm_bf16 calls; these are the launches between them.  An activation is (M * K, channels) float32,
 * channels contiguous and a multiple of 64 (at most 8192), utterance m in the rows [m * K, (m + 1) * K), no halo rows.
 *
 * Global layer norm statistics travel as PARTIALS: for a (M, K, C) tensor, ma_tasnet_stat_parts(K, C) = P workgroups per utterance
 * each leave three float64 - (count, sum, sum of (v - its own mean)^2) of its tile - at part[(m * P + p) * 3].  A consumer joins its
 * utterance's P partials itself in index order; mean = sum / count, var = M2 / count (the mean of (v - mean)^2), normalised value =
 * (v - mean) / sqrt(var + 1e-8), gamma = 1, beta = 0 (conv_tasnet.py:439-463).  No atomics: the same bits from run to run.
 *
 * ma_tasnet_encode_f32: x (M, T) float32, row stride ldx; Wt (L, N) float32 = the transposed encoder weight; L even.
 *   mixture_w[m * K + k, n] = relu(sum_j x[m, k * L/2 + j] * Wt[j, n]),  K = (T - L) / (L / 2) + 1 (floor);  part: P(K, N) partials.
 * ma_prelu_gln_stats: y = x >= 0 ? x : weight[0] * x (weight: one float32 on the device; y may be x), part: the moments of y.
 * ma_gln_dwconv_prelu: z[k, c] = prelu(sum_p Wt[p, c] * n[k + (p - 1) * dilation, c]) with n the normalised y (part_in) and n = 0
 *   outside [0, K) of the SAME utterance; Wt (P, C) float32 = the transposed depthwise weight, P == 3 (else MA_ERR_UNSUPPORTED);
 *   part_out: the moments of z.  z must not be y.
 * ma_gln_apply_bf16: out (M * K, C) bf16 = the normalised y, rounded to nearest even.
 * ma_tasnet_decode_f32: score (M * K, C * N) float32 (channel c * N + n), mixture_w (M * K, N), basis (L, N) float32 (the Dense
 *   weight); frame_k[l] = sum_n relu(score) * mixture_w * basis[l, n].  out (M, C, (K + 1) * L / 2):
 *     MA_TASNET_OVERLAP_PAIRED  out[k * L/2 + j] = frame_k[j] + frame_k[j + L/2], then L / 2 zeros - what the reference's 0 / 1 matrix
 *                               product computes (conv_tasnet.py:113-119, 187) followed by its pad;
 *     MA_TASNET_OVERLAP_TRUE    out[k * L/2 + j] += frame_k[j], j < L: the overlap-add.
 *   L even and <= 64, N % 64 == 0 and <= 768.
 * ma_si_snr_pairwise: source, estimate (B, C, T) float32, lengths (B) int64 -> out (B, C, C) float64, out[b, i, j] = SI-SNR in dB of
 *   estimate i against target j over the first lengths[b] samples, lengths[b] clamped to [0, T] (separation_loss.py:188-216: both
 *   zero-meaned by sum / length; a length of 0 gives 10 log10(EPS) = -80 dB for every pair;
 *   EPS = 1e-8 added to the target energy, to the noise energy and inside the logarithm), everything in float64.
 * All: MA_ERR_INVALID_ARG for a null pointer, a dimension < 1 or a misaligned base (16 bytes), MA_ERR_UNSUPPORTED for a shape outside
 * the above; nothing is launched on a refusal. */
#define MA_TASNET_OVERLAP_PAIRED 0
#define MA_TASNET_OVERLAP_TRUE 1
int32_t ma_tasnet_stat_parts(int64_t K, int32_t C);
int ma_tasnet_encode_f32(const float* x, int64_t M, int64_t T, int64_t ldx, const float* Wt, int32_t L, int32_t N, float* mixture_w,
                         double* part, ma_stream_t stream);
int ma_prelu_gln_stats(const float* x, int64_t M, int64_t K, int32_t C, const float* weight, float* y, double* part,
                       ma_stream_t stream);
int ma_gln_dwconv_prelu(const float* y, int64_t M, int64_t K, int32_t C, const double* part_in, const float* Wt, int32_t P,
                        int32_t dilation, const float* weight, float* z, double* part_out, ma_stream_t stream);
int ma_gln_apply_bf16(const float* y, int64_t M, int64_t K, int32_t C, const double* part, void* out, ma_stream_t stream);
int ma_tasnet_decode_f32(const float* score, const float* mixture_w, int64_t M, int64_t K, int32_t C, int32_t N, const float* basis,
                         int32_t L, int32_t overlap, float* out, ma_stream_t stream);
int ma_si_snr_pairwise(const float* source, const float* estimate, const int64_t* lengths, int64_t B, int32_t C, int64_t T, double* out,
                       ma_stream_t stream);

/* ---- Conv-TasNet training (examples/conv_tasnet/train.py): the launches of the backward between its GEMMs, and the optimizer ---------
 * dX = dY . W is ma_gemm_bf16 on a transposed weight copy (the residual stream's gradient rides in its residual epilogue), dW = dY^T . X
 * is ma_gemm_tn_bf16_f32; in the float32 validation mode both are ma_gemm_x32.  Layout, tiles and the (count, sum, M2) partials as above.
 * The backward of a global layer norm, dx = (dy - mean(dy) - xhat mean(dy xhat)) / sigma, needs two more whole-utterance sums; they
 * travel as part2[(m * P + p) * 2] = (sum(dy), sum(dy * xhat)) of tile p, float64, joined in index order by the consumer.  xhat is
 * recomputed from the saved pre-activation, the PReLU slope and the forward's partials.  Parameter gradients leave as float32 partials,
 * one per workgroup, for ma_reduce_splits_batch_f32.  No atomics: the same bits from run to run.
 *
 * ma_gln_dwconv_prelu_train: ma_gln_dwconv_prelu that also writes `pre`, the depthwise output before its PReLU (same z, same part_out).
 * ma_gln_apply_f32: ma_gln_apply_bf16 with a float32 output.
 * ma_si_snr_grad_f32: grad (B, C, T) float32 = d(-mean_b(sum_j snr[b, perm[b, j], j] / C)) / d estimate in closed float64 form, snr as
 *   ma_si_snr_pairwise computes it (zero-mean over the first lengths[b] samples, the same EPS placement); perm (B, C) int64 on the
 *   device, target j <- estimate perm[b, j], a permutation of 0 .. C - 1 per row (every estimate row is then written exactly once).
 *   grad is exactly 0 at and beyond lengths[b].
 * ma_tasnet_decode_bwd_f32: the backward of ma_tasnet_decode_f32 for both overlaps.  d_out (M, C, (K + 1) L / 2) -> d_score
 *   (M * K, C * N) = d_source_w * mixture_w * (score > 0), d_mixture_w (M * K, N) = sum_c d_source_w * relu(score) (the decoder's share
 *   only), d_basis_part [M * G][L][N] with G = ma_tasnet_decode_bwd_parts(K, C, N, L) (0: unsupported).  L even and <= 64, N % 64 == 0,
 *   L * N <= 12288, C <= 16.
 * ma_tasnet_encode_bwd_f32: d_mixture_w_total = d_mixture_w + gLN backward of d_norm (the gradient at the normalised mixture_w, with
 *   part2 from ma_gln_bwd_stats(d_norm, mixture_w, weight = 1)); d_Ut_part [M * G][L][N] (the order of Wt) = sum over the workgroup's frames of
 *   d_mixture_w_total * (mixture_w > 0) (x) the frame's samples, G = ma_tasnet_encode_bwd_parts(K, N, L).  Same shape limits.
 * ma_gln_bwd_stats: part2 of dy against xhat = gLN(prelu(v, weight[0])) with v's forward partials `part` (weight = 1: no PReLU).
 * ma_gln2_bwd_dwconv: d_h (the gradient at the second gLN's output), d0 (the depthwise output before PReLU, partials part_b of its
 *   PReLU), y0 (the conv1x1 output before PReLU, partials part_a of its PReLU) -> d_u (the gradient at the FIRST gLN's output) through
 *   the gLN backward (part2_h), the PReLU backward and the three dilated taps, each checked against [0, K) of its own utterance;
 *   part2_u = ma_gln_bwd_stats of d_u against y0; d_weight2_part [M * P] (the second slope), d_Wt_part [M * P][3][C] (the taps, the
 *   order of Wt).  C in {64, 128, 256, 512, 1024}; d_u must not be an input.
 * ma_gln1_bwd: d_u, y0 -> out (M * K, C) = the gradient at y0, bf16 (out_bf16 != 0, round to nearest even) or float32;
 *   d_weight_part [M * P] (the first slope).
 * ma_sgd_momentum_f32: nn.SGD as train.py:91-96 builds it.  g = grad + weight_decay * param; momentum > 0: buf = g on the first step
 *   (first_step != 0; buf is then not read), else buf = momentum * buf + g, and param -= lr * buf; momentum == 0: param -= lr * g (buf
 *   may be NULL).  mirror_bf16 (n) bf16, optional: the updated parameters rounded to nearest even.  n % 4 == 0, 16-byte aligned.
 * All: MA_ERR_INVALID_ARG for a null pointer, a dimension < 1 or a misaligned base, MA_ERR_UNSUPPORTED for a shape outside the above;
 * nothing is launched on a refusal. */
int ma_gln_dwconv_prelu_train(const float* y, int64_t M, int64_t K, int32_t C, const double* part_in, const float* Wt, int32_t P,
                              int32_t dilation, const float* weight, float* pre, float* z, double* part_out, ma_stream_t stream);
int ma_gln_apply_f32(const float* y, int64_t M, int64_t K, int32_t C, const double* part, float* out, ma_stream_t stream);
int ma_si_snr_grad_f32(const float* source, const float* estimate, const int64_t* lengths, const int64_t* perm, int64_t B, int32_t C,
                       int64_t T, float* grad, ma_stream_t stream);
int32_t ma_tasnet_decode_bwd_parts(int64_t K, int32_t C, int32_t N, int32_t L);
int ma_tasnet_decode_bwd_f32(const float* d_out, const float* score, const float* mixture_w, int64_t M, int64_t K, int32_t C, int32_t N,
                             const float* basis, int32_t L, int32_t overlap, float* d_score, float* d_mixture_w, float* d_basis_part,
                             ma_stream_t stream);
int32_t ma_tasnet_encode_bwd_parts(int64_t K, int32_t N, int32_t L);
int ma_tasnet_encode_bwd_f32(const float* x, int64_t M, int64_t T, int64_t ldx, const float* mixture_w, const double* part,
                             const float* d_norm, const double* part2, const float* d_mixture_w, int32_t L, int32_t N, float* d_Ut_part,
                             ma_stream_t stream);
int ma_gln_bwd_stats(const float* dy, const float* v, int64_t M, int64_t K, int32_t C, const double* part, const float* weight,
                     double* part2, ma_stream_t stream);
int ma_gln2_bwd_dwconv(const float* d_h, const float* d0, const float* y0, int64_t M, int64_t K, int32_t C, const double* part_a,
                       const double* part_b, const double* part2_h, const float* weight1, const float* weight2, const float* Wt,
                       int32_t P, int32_t dilation, float* d_u, double* part2_u, float* d_weight2_part, float* d_Wt_part,
                       ma_stream_t stream);
int ma_gln1_bwd(const float* d_u, const float* y0, int64_t M, int64_t K, int32_t C, const double* part_a, const double* part2_u,
                const float* weight, void* out, int32_t out_bf16, float* d_weight_part, ma_stream_t stream);
int ma_sgd_momentum_f32(float* param, const float* grad, float* buf, int64_t n, float lr, float momentum, float weight_decay,
                        int32_t first_step, void* mirror_bf16, ma_stream_t stream);

/* ---- Bidirectional LSTM layer, inference (mindaudio/models/deepspeech2.py:119-187: nn.LSTM(bidirectional=True, has_bias=True), the
 * two directions summed) --------------------------------------------------------------------------------------------------------------
 * Cell, PyTorch gate order i, f, g, o:  gates = x W_ih^T + b_ih + h W_hh^T + b_hh,  c' = sigmoid(f) c + sigmoid(i) tanh(g),
 * h' = sigmoid(o) tanh(c'),  h_0 = c_0 = 0.  The reverse direction walks t = T - 1 .. 0 and writes at index t; there are no lengths:
 * both directions run over all T frames.  out[t] = h_fwd[t] + h_bwd[t].
 * Rounding points: x, W_ih, W_hh and the h that is fed back are bf16 MFMA operands (round to nearest even); projections, gate sums, c
 * and the output are float32, accumulation is float32; out_bf16 is the rounding of out_f32.  No atomics: the same bits run to run.
 *
 * ma_lstm_pack_f32: one layer's weights, both directions stacked: w_ih (2, 4H, K), w_hh (2, 4H, H), b_ih / b_hh (2, 4H) float32 ->
 *   wih_bf16 (2, 4H, Kpad) bf16 with zero columns K .. Kpad - 1, whh_packed (2 * 4H * H bf16, in the step kernel's fragment order),
 *   bias (2, 4H) float32 = b_ih + b_hh.  Outputs 16-byte aligned.
 * ma_lstm_bidir_bf16: x (T, B, Kpad) bf16 -> out_f32 (T, B, H) float32 and out_bf16 (T, B, H) bf16 (NULL: left out).
 *   Per chunk of time_chunk steps: one ma_gemm_bf16 per direction (the input projection, float32, bias folded in), then ONE LAUNCH PER
 *   TIME STEP from a host loop inside this call - each serves both directions and does the h W_hh^T product on MFMA, the gate
 *   arithmetic, the c update and the stores; stream order is the only synchronisation between steps (no persistent kernel, no
 *   inter-workgroup waiting).  dir_mask: 1 forward only, 2 reverse only (the other half counts as zero), 3 both.
 *   c_final (2, B, H) float32, optional: the cell state after the last step of each direction.
 *   workspace >= ma_lstm_workspace_bytes(T, B, H, time_chunk), 16-byte aligned: MA_ERR_WORKSPACE otherwise.
 * Shapes: T >= 1, B >= 1 (rows beyond B are never read), H % 64 == 0 (64 .. 4096), Kpad % 64 == 0: MA_ERR_UNSUPPORTED otherwise;
 * MA_ERR_INVALID_ARG for a null or misaligned pointer, a size < 1 or a dir_mask outside 1 .. 3; a failed launch returns MA_ERR_LAUNCH
 * and ends the loop. */
int64_t ma_lstm_workspace_bytes(int64_t T, int64_t B, int32_t H, int64_t time_chunk);
int ma_lstm_pack_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int32_t K, int32_t Kpad, int32_t H,
                     void* wih_bf16, void* whh_packed, float* bias, ma_stream_t stream);
int ma_lstm_bidir_bf16(const void* x, int64_t T, int64_t B, int32_t Kpad, int32_t H, const void* wih_bf16, const void* whh_packed,
                       const float* bias, int32_t dir_mask, int64_t time_chunk, float* out_f32, void* out_bf16, float* c_final,
                       void* workspace, int64_t workspace_bytes, ma_stream_t stream);

/* ---- Bidirectional LSTM layer, training: the forward that keeps a tape, and backward through time -------------------------------------
 * ma_lstm_bidir_train_bf16: ma_lstm_bidir_bf16 with the same operands, schedule and launches (the step kernels' taping
 *   instantiations): out_f32, out_bf16 and c_final have the SAME BITS.  It also fills `tape`, ma_lstm_train_tape_bytes(T, B, H) bytes,
 *   16-byte aligned (MA_ERR_WORKSPACE when tape_bytes is less):
 *     act (2, T, 5, B, H) float32 at offset 0: per direction and frame the planes i, f, g, o - the ACTIVATED gates - and c_t;
 *     h   (2, T, B, H) bf16 at ma_lstm_train_tape_h_offset(T, B, H): the h_t that was fed back (the MFMA operand of the next step).
 *   A direction outside dir_mask leaves its half untouched.  (T = 625, B = 64, H = 1024: 1.80 GB.)
 * ma_lstm_pack_bwd_f32: w_hh (2, 4H, H) float32 -> whh_bwd_packed, 2 * 4H * H bf16 in the backward step's fragment order
 *   (csrc/lstm_common.h: per slice of 16 hidden units the k-steps over gate * H + unit), 16-byte aligned.
 * ma_lstm_bidir_bwd_bf16: dout (T, B, H) float32 = dL/d(out); it feeds both directions, out being their sum.  -> dgates
 *   (2, T, B, 4H) bf16, gate order i, f, g, o: the gradient with respect to the PRE-ACTIVATION gate sums per direction; the half of a
 *   direction outside dir_mask is set to zero.  ONE LAUNCH PER TIME STEP from a host loop inside the call, each serving both
 *   directions (step s: t = T - 1 - s forward, t = s reverse); stream order is the only synchronisation, no atomics: the same bits
 *   run to run.  Per step: dh = dout[t] + dgates_next . W_hh (MFMA, float32 accumulation), th = tanh(c_t),
 *     do = dh th o (1 - o),  dc = dh o (1 - th^2) + dc_next,  di = dc g i (1 - i),  dg = dc i (1 - g^2),  df = dc c_{t-1} f (1 - f)
 *     with c_{-1} = 0,  dc_next <- dc f.
 *   Rounding points: dgates -> bf16 (round to nearest even) as the stored result and as the next step's MFMA operand, W_hh -> bf16 in
 *   the pack; dout, dh, dc, the tape and every factor are float32.  The parameter and input gradients follow from dgates by the
 *   library's products: dW_ih = ma_gemm_tn_bf16_f32(dgates[dir], x) with colsum = db_ih = db_hh, dW_hh the same against the tape's h
 *   shifted by one frame (B rows), dx = sum over dir of ma_gemm_bf16(dgates[dir], W_ih[dir]^T).
 *   workspace >= ma_lstm_bwd_workspace_bytes(B, H), 16-byte aligned; it or the tape too short: MA_ERR_WORKSPACE.
 * Shapes and error codes as for ma_lstm_bidir_bf16. */
int64_t ma_lstm_train_tape_bytes(int64_t T, int64_t B, int32_t H);
int64_t ma_lstm_train_tape_h_offset(int64_t T, int64_t B, int32_t H);
int ma_lstm_bidir_train_bf16(const void* x, int64_t T, int64_t B, int32_t Kpad, int32_t H, const void* wih_bf16, const void* whh_packed,
                             const float* bias, int32_t dir_mask, int64_t time_chunk, float* out_f32, void* out_bf16, float* c_final,
                             void* tape, int64_t tape_bytes, void* workspace, int64_t workspace_bytes, ma_stream_t stream);
int ma_lstm_pack_bwd_f32(const float* w_hh, int32_t H, void* whh_bwd_packed, ma_stream_t stream);
int64_t ma_lstm_bwd_workspace_bytes(int64_t B, int32_t H);
int ma_lstm_bidir_bwd_bf16(const float* dout, int64_t T, int64_t B, int32_t H, const void* tape, int64_t tape_bytes,
                           const void* whh_bwd_packed, int32_t dir_mask, void* dgates, void* workspace, int64_t workspace_bytes,
                           ma_stream_t stream);

/* ---- DeepSpeech2 (mindaudio/models/deepspeech2.py) outside its LSTM layers and GEMMs ---------------------------------------------------
 * ma_ds2_conv1_bf16: Conv2d(1 -> 32, (41, 11), stride (2, 2), pad (20, 5), no bias) + BatchNorm2d in affine form + tanh.
 *   x (B, F, T) float32; wt (451, 32) float32 = the weight transposed to [frequency tap * 11 + time tap][channel]; scale / shift (32).
 *   out: the (T1 + 10, B, Fpad, 32) bf16 activation of the second convolution (time-major, channel-last), F1 = (F - 1) / 2 + 1,
 *   T1 = (T - 1) / 2 + 1; only frames 5 .. 5 + T1 - 1 and frequency rows 10 .. 10 + F1 - 1 are written, the caller keeps the rest zero.
 *   float32 accumulation in tap order.  F <= 256, B <= 65535, Fpad >= F1 + 20: MA_ERR_UNSUPPORTED otherwise.
 * ma_ds2_softmax_f32: probs (B, T, C) = softmax over the C classes of logits (T, B, row stride ld): PredictWithSoftmax
 *   (examples/deepspeech2/eval.py:17-33). */
int ma_ds2_conv1_bf16(const float* x, int64_t B, int32_t F, int64_t T, const float* wt, const float* scale, const float* shift,
                      int32_t Fpad, void* out, ma_stream_t stream);
int ma_ds2_softmax_f32(const float* logits, int64_t ld, int64_t T, int64_t B, int32_t C, float* probs, ma_stream_t stream);

/* ---- DeepSpeech2's convolution front end in TRAINING mode (csrc/deepspeech2_train.hip): conv1, conv2 and both BatchNorm2d trained ----
 * Channel-last everywhere, 32 channels, channel = column mod 32.  Every statistic is summed in double per thread, per workgroup and
 * over the workgroups' partials ((a | b) of 64 doubles each), always in a fixed order; no atomics: the same bits run to run.
 * ma_ds2_conv1_raw_f32: ma_ds2_conv1_bf16's convolution without its epilogue: y1 (T1, B, F1, 32) float32, the accumulators themselves,
 *   and ma_ds2_conv1_raw_parts(B, T) partials (sum | sum of squares).
 * ma_ds2_bn_stats_f32: the same partials, ma_ds2_stats_parts(n) of them, of n float32 values (n % 32 == 0, 16-byte aligned).
 * ma_ds2_bn_finalize_f32: stats (96) = mean | 1 / sqrt(biased variance + eps) | biased variance over `count` values per channel;
 *   mean_out / var_out (both or neither) = (1 - momentum) * mean_in / var_in + momentum * (mean, variance * count / (count - 1)):
 *   the moving statistics are never updated in place.
 * ma_ds2_bn_tanh_fwd_bf16: out[r * ldo + c] = bf16(tanh(fma(gamma, (y[r, c] - mean) * rstd, beta))) for y (rows, cols) contiguous,
 *   cols % 32 == 0, ldo % 4 == 0; nothing else of `out` is touched.
 * ma_ds2_bn_tanh_bwd_f32: the backward of that stage from the raw y and dout (rows, row stride ldd) float32 in three launches:
 *   dn = dout (1 - a^2) with a recomputed as above and its partials (sum dn | sum dn xhat); their join bsum (128) = d_beta | d_gamma |
 *   mean dn | mean dn xhat, also stored to d_gamma / d_beta (32 each, optional); dz = gamma rstd (dn - mean dn - xhat mean dn xhat)
 *   to out[r * ldo + c], bf16 (out_bf16 != 0) or float32.  workspace >= ma_ds2_bn_tanh_bwd_workspace_bytes(rows, cols), 8-byte aligned.
 * ma_ds2_conv1_dw_f32: dw (32, 451) = sum over (b, f1, t1) of dz1[t1, b, f1, c] * x[b, 2 f1 + kf - 20, 2 t1 + kt - 5] (zero outside x),
 *   dz1 (T1, B, F1, 32) float32.  A workgroup walks frames_per_wg frames (0: ceil(B T1 / 1024)) with float32 fused multiply-adds, a
 *   chain of frames_per_wg * F1 per output; the ma_ds2_conv1_dw_parts partials are added in double in partial order.
 *   workspace >= parts * 451 * 32 * 4 bytes, 16-byte aligned.
 * ma_ds2_commit_f32: dst[i] = src[i], i < n, unless overflow[0] != 0 (the moving statistics of a step that is not skipped).
 * Shapes as ma_ds2_conv1_bf16: F <= 256, B <= 65535. */
int32_t ma_ds2_conv1_raw_parts(int64_t B, int64_t T);
int ma_ds2_conv1_raw_f32(const float* x, int64_t B, int32_t F, int64_t T, const float* wt, float* y1, double* partials,
                         ma_stream_t stream);
int32_t ma_ds2_stats_parts(int64_t n);
int ma_ds2_bn_stats_f32(const float* y, int64_t n, double* partials, ma_stream_t stream);
int ma_ds2_bn_finalize_f32(const double* partials, int32_t nparts, int64_t count, float eps, float momentum, const float* mean_in,
                           const float* var_in, float* mean_out, float* var_out, float* stats, ma_stream_t stream);
int ma_ds2_bn_tanh_fwd_bf16(const float* y, int64_t rows, int32_t cols, const float* stats, const float* gamma, const float* beta,
                            void* out, int64_t ldo, ma_stream_t stream);
int64_t ma_ds2_bn_tanh_bwd_workspace_bytes(int64_t rows, int32_t cols);
int ma_ds2_bn_tanh_bwd_f32(const float* y, const float* dout, int64_t ldd, int64_t rows, int32_t cols, const float* stats,
                           const float* gamma, const float* beta, void* out, int64_t ldo, int32_t out_bf16, float* bsum, float* d_gamma,
                           float* d_beta, void* workspace, int64_t workspace_bytes, ma_stream_t stream);
int32_t ma_ds2_conv1_dw_parts(int64_t B, int64_t T, int32_t frames_per_wg);
int ma_ds2_conv1_dw_f32(const float* x, int64_t B, int32_t F, int64_t T, const float* dz1, int32_t frames_per_wg, float* dw,
                        void* workspace, int64_t workspace_bytes, ma_stream_t stream);
int ma_ds2_commit_f32(float* dst, const float* src, int32_t n, const int32_t* overflow, ma_stream_t stream);

/* ---- Layer-pipelined unidirectional LSTM stack, inference (mindaudio/models/tasnet.py:106-108: nn.LSTM(N, hidden_size, num_layers,
 * bidirectional=False)) -----------------------------------------------------------------------------------------------------------------
 * The cell and its gate order are those of the block above; h_0 = c_0 = 0 in every layer; layer l >= 1 reads layer l - 1's h.
 * Rounding points: x, W_ih, W_hh and every h that feeds a product (a layer's own h_{t-1} and the lower layer's h_t) are bf16 MFMA
 * operands (round to nearest even); gate sums, c, the output and h_final are float32, accumulation is float32 in a fixed order;
 * out_bf16 is the rounding of out_f32.  No atomics: the same bits run to run.
 *
 * ma_lstm_stack_pack_f32: ONE layer's weights: w_ih (4H, K), w_hh (4H, H), b_ih / b_hh (4H) float32 -> packed: 4H * (Kpad + H) bf16
 *   holding [W_ih | W_hh] along K in the step kernel's fragment order [slice of 16 units][k-step of 32][gate][lane][8], the columns
 *   K .. Kpad - 1 zero; bias (4H) float32 = b_ih + b_hh.  Layer 0 has K = the input width; a layer above it has K = Kpad = H.
 *   Outputs 16-byte aligned.
 * ma_lstm_stack_bf16: x (T, B, Kpad) bf16 -> out_f32 (T, B, H) float32 and out_bf16 (T, B, H) bf16 (NULL: left out) of the LAST layer.
 *   packed / bias: HOST arrays of n_layers device pointers.  A host loop inside this call walks the diagonals d = t + l =
 *   0 .. T + n_layers - 2, ONE LAUNCH PER DIAGONAL that serves every layer active on it (layer l runs t = d - l):
 *   gates = [x_t | h_{t-1}] . [W_ih | W_hh]^T + bias in one K loop on MFMA, then the cell.  Stream order is the only synchronisation
 *   between launches (no persistent kernel, no inter-workgroup waiting).  Per layer the workspace holds two bf16 images of h, written
 *   at parity d & 1 and read at parity (d - 1) & 1, and one float32 c.
 *   h_final / c_final (n_layers, B, H) float32, optional: h and c after the last step of each layer.
 *   workspace >= ma_lstm_stack_workspace_bytes(T, B, H, n_layers), 16-byte aligned: MA_ERR_WORKSPACE otherwise.
 * Shapes: T >= 1, B >= 1 (rows beyond B are never read), H % 64 == 0 (64 .. 4096), Kpad % 64 == 0, n_layers 1 .. 8: MA_ERR_UNSUPPORTED
 * otherwise; MA_ERR_INVALID_ARG for a null or misaligned pointer or a size < 1; a failed launch returns MA_ERR_LAUNCH and ends the
 * loop. */
int64_t ma_lstm_stack_workspace_bytes(int64_t T, int64_t B, int32_t H, int32_t n_layers);
int ma_lstm_stack_pack_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int32_t K, int32_t Kpad, int32_t H,
                           void* packed, float* bias, ma_stream_t stream);
int ma_lstm_stack_bf16(const void* x, int64_t T, int64_t B, int32_t Kpad, int32_t H, int32_t n_layers, const void* const* packed,
                       const float* const* bias, float* out_f32, void* out_bf16, float* h_final, float* c_final, void* workspace,
                       int64_t workspace_bytes, ma_stream_t stream);

/* ---- TasNet (mindaudio/models/tasnet.py) outside its LSTM stack and fc GEMM, float32 ---------------------------------------------------
 * ma_tasnet_gated_encode_f32: mixture (B, K, L) float32.  Per segment row (b, k): norm_coef[b, k] = sqrt(sum x^2); xn = x / (norm_coef +
 *   1e-8); mixture_w[b, k, n] = relu(sum_j xn[j] Ut[j, n] + bU[n]) * sigmoid(sum_j xn[j] Vt[j, n] + bV[n]) with Ut, Vt (L, N) the
 *   transposed Conv1d(L, N, 1) weights; then LayerNorm over N (mean and biased variance of the row, (v - mean) / sqrt(var + ln_eps) *
 *   gamma + beta) stored as bf16 into xin (K, B, Kpad), row k * B + b, columns 0 .. N - 1: the LSTM stack's time-major input.  The
 *   columns N .. Kpad - 1 are never written (the caller zeroes them once).  L <= 64, N <= 1024: MA_ERR_UNSUPPORTED otherwise.
 * ma_tasnet_mask_decode_f32: score (K * B, nspk * N) float32, row k * B + b, row stride ld_score, column s * N + n (the fc output).
 *   mask = softmax over the nspk speakers per (row, n); source_w = mixture_w[b, k, n] * mask;
 *   out[b, s, k, l] = (sum_n source_w[s, n] basis[l, n] + bias[l]) * norm_coef[b, k] (the reference multiplies the bias too), out
 *   (B, nspk, K, L).  nspk 1 .. 4, L <= 64, N <= 1024: MA_ERR_UNSUPPORTED otherwise.
 * Both: MA_ERR_INVALID_ARG for a null pointer, a dimension < 1 or a misaligned base (16 bytes); fixed summation order. */
int ma_tasnet_gated_encode_f32(const float* mixture, int64_t B, int64_t K, int32_t L, int32_t N, const float* Ut, const float* bU,
                               const float* Vt, const float* bV, const float* gamma, const float* beta, float ln_eps, float* mixture_w,
                               float* norm_coef, void* xin, int32_t Kpad, ma_stream_t stream);
int ma_tasnet_mask_decode_f32(const float* score, int64_t ld_score, const float* mixture_w, const float* norm_coef, int64_t B, int64_t K,
                              int32_t nspk, int32_t N, const float* basis, const float* bias, int32_t L, float* out, ma_stream_t stream);

/* ---- WaveGrad vocoder (mindaudio/models/wavegrad/wavegrad_v190.py, examples/wavegrad/reverse.py) -----------------------------------------
 * Activations are time-major, channel-last float32 (B, T_l, C), compact.  bf16 exists only as an MFMA operand: (B, T_l + 2 * halo, Cpad)
 * with zero halo rows around every utterance and zero columns C .. Cpad - 1 (Cpad % 64 == 0), the layout of ma_conv1d_taps_bf16.  No
 * atomics, no cross-workgroup waiting: the same bits from run to run.  All: every argument check comes before any HIP call; 16-byte
 * aligned bases; nothing allocates or synchronises.
 *
 * ma_wavegrad_init_conv_f32: Conv1d(1 -> C0, `taps` odd <= 7, pad same, bias) on audio (B, T) float32, float32 weights wt (taps, C0)
 *   (transposed), fma chain in tap order starting from the bias -> out (B, T, C0).  Taps outside the utterance read zero.  C0 % 4 == 0.
 * ma_wavegrad_pack_bf16: the operand producer in front of every MFMA product.  For output row t < T_in * f of utterance b, channel c:
 *     v = x[b, t / f, c]                                  x (B, T_in, C) float32; f >= 1 is nearest-neighbour repetition
 *     res[b, t, c] = v * res_mul                           (res != NULL: (B, T_in * f, C) float32)
 *     v = fma(scale, v, shift) * (1 / sqrt 2)              (film != NULL: a (B * T_in * f, >= 2 C) float32 matrix, row stride ld_film,
 *                                                           shift = columns 0 .. C - 1, scale = columns C .. 2 C - 1)
 *     v = v >= 0 ? v : slope * v                           (slope = 1: a plain cast)
 *     v += enc[b * ld_enc + c]                             (enc != NULL; ld_enc = 0 broadcasts one row over the batch)
 *     v *= mul;  out = bf16(v), round to nearest even
 *   out (B, T_in * f + 2 * halo, Cpad) bf16: halo rows and the columns C .. Cpad - 1 are written as zeros on every call; halo >= 0.
 *   out may be NULL when res is given.  C % 8 == 0, Cpad % 64 == 0, Cpad >= C, ld_film % 4 == 0, ld_enc % 4 == 0: MA_ERR_UNSUPPORTED
 *   otherwise.
 * ma_wavegrad_last_conv_update_f32: Conv1d(C -> 1, `taps` odd <= 7, pad same, bias) on x (B, T, C) float32 with w (taps, C) float32,
 *   fused with the update of reverse.py:116-123:  pred = conv(x);  audio_out = c1 * (audio_in - c2 * pred) (+ sigma * noise when noise
 *   != NULL).  pred (B, T) is stored when non-NULL; audio_out may be NULL (then audio_in and noise are not read) when pred is given;
 *   audio_out == audio_in is allowed.  C % 4 == 0, B <= 65535. */
int ma_wavegrad_init_conv_f32(const float* audio, int64_t B, int64_t T, const float* wt, const float* bias, int32_t taps, int32_t C0,
                              float* out, ma_stream_t stream);
int ma_wavegrad_pack_bf16(const float* x, int64_t B, int64_t T_in, int32_t f, int32_t C, int32_t Cpad, int32_t halo, const float* film,
                          int64_t ld_film, const float* enc, int64_t ld_enc, float slope, float mul, void* out, float* res,
                          float res_mul, ma_stream_t stream);
int ma_wavegrad_last_conv_update_f32(const float* x, int64_t B, int64_t T, int32_t C, const float* w, const float* bias, int32_t taps,
                                     const float* audio_in, const float* noise, float c1, float c2, float sigma, float* audio_out,
                                     float* pred, ma_stream_t stream);

/* One launch (B launches for the MFMA products: one per utterance) of a network evaluation.  Buffers are byte offsets into ONE
 * workspace; MA_WAVEGRAD_BUF_NONE = absent, _AUDIO = the call's audio (B, T), _MEL = the call's spectrogram (B, frames, n_mels) float32
 * (time-major).  T = the rows per utterance of the op's OUTPUT.
 *   MA_WAVEGRAD_OP_INIT  in (AUDIO) -> out (B, T, N) float32; w = wt (taps, N) float32
 *   MA_WAVEGRAD_OP_PACK  in x (B, T / f, C) float32, in2 = film matrix (row stride ld_film) or NONE, enc_off >= 0: the step's encoding
 *                        row + enc_off; -> out (B, T + 2 halo, Cpad) bf16 or NONE, out2 = res or NONE
 *   MA_WAVEGRAD_OP_CONV  ma_conv1d_taps_bf16 per utterance on in (B, T + 2 halo, Cpad) bf16, w (N, taps, Cpad) bf16, bias, alpha,
 *                        residual (B, T, N) float32 or NONE -> out (B, T, N) float32, or bf16 when out_bf16 (N % 64 == 0 then)
 *   MA_WAVEGRAD_OP_DOWN  the kernel = stride = f convolution as ma_gemm_bf16 per utterance on in (B, T * f + 2 halo, Cpad) bf16:
 *                        A = the utterance's first real row, lda = K = f * Cpad, M = T; w (N, f, Cpad) bf16 -> out (B, T, N) float32
 *   MA_WAVEGRAD_OP_LAST  ma_wavegrad_last_conv_update_f32 on in (B, T, C) float32, w (taps, C) float32
 * `once` ops do not depend on the step (first_conv of the spectrogram): ma_wavegrad_reverse runs them once per call. */
enum { MA_WAVEGRAD_OP_INIT = 0, MA_WAVEGRAD_OP_PACK = 1, MA_WAVEGRAD_OP_CONV = 2, MA_WAVEGRAD_OP_DOWN = 3, MA_WAVEGRAD_OP_LAST = 4 };
#define MA_WAVEGRAD_BUF_NONE (-1)
#define MA_WAVEGRAD_BUF_AUDIO (-2)
#define MA_WAVEGRAD_BUF_MEL (-3)
typedef struct ma_wavegrad_op {
  int32_t kind, once;
  int64_t in, in2, out, out2, residual; /* byte offsets into the workspace (multiples of 16) or MA_WAVEGRAD_BUF_* */
  const void* w;                        /* device */
  const float* bias;                    /* device */
  int64_t T, ld_film;
  int32_t C, Cpad, N, taps, dilation, f, halo, out_bf16, enc_off, reserved;
  float slope, mul, res_mul, alpha;
} ma_wavegrad_op_t;

/* The network for one (B, frames) shape: plain data, filled by the caller once per shape.  T = hop * frames; enc_dim = the floats
 * of one step's positional-encoding row (the sum over the FiLM levels). */
typedef struct ma_wavegrad_plan {
  int32_t n_ops, enc_dim;
  int64_t B, T, frames, n_mels;
  const ma_wavegrad_op_t* ops; /* host */
} ma_wavegrad_plan_t;

/* Bytes of workspace the plan's offsets reach (the largest offset + extent over its ops); a negative MA_ERR_* for a plan that
 * ma_wavegrad_forward would refuse (an unknown kind, a misaligned or missing buffer, a halo smaller than (taps / 2) * dilation, ...). */
int64_t ma_wavegrad_workspace_bytes(const ma_wavegrad_plan_t* plan);

/* ma_wavegrad_forward: one network evaluation, a host loop over the plan's ops inside one call.  audio (B, T), mel (B, frames, n_mels),
 *   enc (B or 1, enc_dim) float32 with row stride ld_enc (0: one row for the whole batch) -> pred (B, T) float32.
 * ma_wavegrad_reverse: iterations m = first_step .. first_step + n_steps - 1 of the S-step loop of reverse.py:114-123 back to back, n =
 *   S - 1 - m:  pred = network(audio, enc_table[n]);  audio = c1[n] * (audio - c2[n] * pred) + (n > 0 ? sigma[n] * noise[m - first_step]
 *   : 0), audio (B, T) updated in place.  c1, c2, sigma: HOST arrays [S]; enc_table (S, enc_dim) and noise (n_steps, B, T; the entry of
 *   n == 0 is never read and may be missing) on the device.  Between its first and its last launch there is no host synchronisation,
 *   no read-back and no allocation; the `once` ops run once per call.
 * Both: MA_ERR_WORKSPACE when workspace_bytes < ma_wavegrad_workspace_bytes(plan); a failed launch returns MA_ERR_LAUNCH and ends
 * the call. */
int ma_wavegrad_forward(const ma_wavegrad_plan_t* plan, const float* audio, const float* mel, const float* enc, int64_t ld_enc,
                        float* pred, void* workspace, int64_t workspace_bytes, ma_stream_t stream);
int ma_wavegrad_reverse(const ma_wavegrad_plan_t* plan, float* audio, const float* mel, const float* enc_table, const float* c1,
                        const float* c2, const float* sigma, const float* noise, int32_t S, int32_t first_step, int32_t n_steps,
                        void* workspace, int64_t workspace_bytes, ma_stream_t stream);

/* ---- WaveGrad training (examples/wavegrad/train.py: L1 loss, MyTrainOneStepCell's unscale / clip_by_global_norm / nn.Adam) ---------------
 * The backward pass walks the forward's op list in reverse around existing products: the gradient of a CONV / DOWN output becomes an
 * operand image through ma_wavegrad_pack_bf16 (slope 1, mul = the convolution's alpha); dX is ma_conv1d_taps_bf16 / ma_gemm_bf16 on the
 * transposed weight copies of ma_wavegrad_weights_bf16, dW ma_gemm_tn_bf16_f32 per tap.  The entries below are what sits between them.
 * The rules of the WaveGrad section hold: every argument check comes before any HIP call, 16-byte aligned bases, nothing allocates or
 * synchronises, no atomics - the same bits from run to run.  Sums over per-workgroup float32 partials are left to
 * ma_reduce_splits_batch_f32 (the caller's item table).
 *
 * ma_wavegrad_l1_last_bwd_f32: the L1 loss and the backward of last_conv (Conv1d(C -> 1, `taps` odd <= 7, pad same)) in one launch, plus
 *   a one-workgroup launch that joins the loss.  pred, noise (B, T); x (B, T, C) the convolution's input; w (taps, C) float32.
 *     loss[0] = mean |pred - noise| as float64: |float32 difference| summed in float64, one partial per workgroup (loss_part, >=
 *       ma_wavegrad_last_bwd_parts(B, T) doubles), joined in a fixed order;
 *     g[b, t] = sign(pred - noise) * loss_scale / (B T), sign(0) = 0                                           (B, T) float32
 *     dx[b, t, c] = sum_j g[b, t - (j - taps/2)] w[j, c], taps outside the utterance are zero                    (B, T, C) float32, stored
 *     wpart[p * pstride + j * C + c] = workgroup p's sum of g[b, t] x[b, t + j - taps/2, c];  wpart[p * pstride + taps * C] = its sum of g
 *   p < ma_wavegrad_last_bwd_parts(B, T); pstride >= taps * C + 1, a multiple of 4.  C % 4 == 0, C <= 1024, B <= 65535.
 * ma_wavegrad_pack_bwd_f32: the backward of ma_wavegrad_pack_bf16 / ma_wavegrad_pack_f32.  dop = the gradient with respect to the operand
 *   values, float32 (B * T_in * f rows of >= C floats, row stride ld_dop; NULL: the op had no operand output); x, film, slope, mul, f,
 *   res_mul as the forward got them; dres = the gradient of the res side output (B, T_in * f, C) or NULL.  Per output row and channel,
 *   with v = x[b, t / f, c] and pre = the forward's value in front of the LeakyReLU recomputed in the forward's fma order:
 *     g = dop * mul * (pre >= 0 ? 1 : slope)
 *     film:  dshift = g / sqrt 2,  dscale = g * v / sqrt 2  -> dfilm (row stride ld_dfilm, shift | scale as the film matrix; stored, or
 *            added to what is there when acc_film != 0);  g = g * scale / sqrt 2
 *     g += dres * res_mul
 *   dx[b, t / f, c] = (acc_dx ? dx : 0) + the sum over the f repeated rows in row order.  The encoding has no gradient.  dx or dfilm may
 *   be NULL.  C % 4 == 0, strides % 4 == 0.
 * ma_wavegrad_init_conv_bwd_f32: the parameter gradients of ma_wavegrad_init_conv_f32 as per-workgroup partials: part[p * (taps + 1) * C0
 *   + j * C0 + c] = sum of dout[b, t, c] audio[b, t + j - taps/2], and behind the taps [.. + taps * C0 + c] = sum of dout[b, t, c];
 *   p < ma_wavegrad_init_bwd_parts(B, T).  C0 % 4 == 0, C0 <= 1024.
 * ma_wavegrad_sumsq_f64: part[p] = float64 partial of sum g^2, p < ma_wavegrad_sumsq_parts(n) (<= 1024).  n % 4 == 0.
 * ma_wavegrad_clip_adam_f32: one launch over one flat parameter buffer.  Every workgroup joins the partials in the same order;
 *   norm = sqrt(sum) / loss_scale (the norm after the reference's unscaling; stored as float32 in norm[0]); a non-finite norm sets
 *   overflow[0] = 1 and leaves param, m and v untouched; else overflow[0] = 0 and, with factor = clip / max(norm, clip)
 *   (ops.clip_by_global_norm), ma_adam_f32's update on g = (grad / loss_scale) * factor.  n % 4 == 0.
 * ma_wavegrad_weights_bf16: the bf16 operand copies of every convolution from the float32 masters (N, taps, C) in ONE launch; items /
 *   block_item are DEVICE arrays, workgroup b handles elements [256 (b - first_block), + 256) of item block_item[b]'s Npad * taps * Cpad.
 *     fwd (rows_fwd, taps, Cpad): the forward operand, zero columns C .. Cpad - 1 and zero rows N .. rows_fwd - 1 (rows_fwd <= Npad);
 *     rev, mode 0: (C, taps, Npad) with rev[c, taps - 1 - j, n] = w[n, j, c] - the weights of the input-gradient convolution;
 *          mode 1: (taps * Cpad, Npad) with rev[j * Cpad + c, n] = w[n, j, c] - the transposed matrix of a kernel = stride convolution.
 *   Either may be NULL.  Round to nearest even, as ma_cast_f32_bf16.
 * ma_wavegrad_pack_f32: ma_wavegrad_pack_bf16 with a float32 image (B, T_in * f + 2 * halo, C) and no padded columns: the operand
 *   producer of the float32 validation mode (products through ma_gemm_x32).  C % 4 == 0. */
typedef struct ma_wavegrad_weight_item {
  const float* src;
  void* fwd;
  void* rev;
  int32_t N, taps, C, Cpad, Npad, rows_fwd, mode, first_block;
} ma_wavegrad_weight_item_t;
int32_t ma_wavegrad_last_bwd_parts(int64_t B, int64_t T);
int32_t ma_wavegrad_init_bwd_parts(int64_t B, int64_t T);
int32_t ma_wavegrad_sumsq_parts(int64_t n);
int ma_wavegrad_l1_last_bwd_f32(const float* pred, const float* noise, const float* x, int64_t B, int64_t T, int32_t C, const float* w,
                                int32_t taps, float loss_scale, float* g, float* dx, float* wpart, int64_t pstride, double* loss_part,
                                double* loss, ma_stream_t stream);
int ma_wavegrad_pack_bwd_f32(const float* dop, int64_t ld_dop, const float* x, int64_t B, int64_t T_in, int32_t f, int32_t C,
                             const float* film, int64_t ld_film, float slope, float mul, const float* dres, float res_mul, float* dx,
                             int32_t acc_dx, float* dfilm, int64_t ld_dfilm, int32_t acc_film, ma_stream_t stream);
int ma_wavegrad_init_conv_bwd_f32(const float* dout, const float* audio, int64_t B, int64_t T, int32_t taps, int32_t C0, float* part,
                                  ma_stream_t stream);
int ma_wavegrad_sumsq_f64(const float* g, int64_t n, double* part, ma_stream_t stream);
int ma_wavegrad_clip_adam_f32(float* param, const float* grad, float* m, float* v, int64_t n, const double* part, int32_t n_parts,
                              float loss_scale, float clip, float lr_t, float beta1, float beta2, float eps, int32_t* overflow,
                              float* norm, ma_stream_t stream);
int ma_wavegrad_weights_bf16(const ma_wavegrad_weight_item_t* items, const int32_t* block_item, int32_t n_blocks, ma_stream_t stream);
int ma_wavegrad_pack_f32(const float* x, int64_t B, int64_t T_in, int32_t f, int32_t C, int32_t halo, const float* film, int64_t ld_film,
                         const float* enc, int64_t ld_enc, float slope, float mul, float* out, float* res, float res_mul,
                         ma_stream_t stream);

/* ---- FastSpeech2 inference (mindaudio/models/fastspeech2/, mindaudio/models/transformer/) -------------------------------------------------
 * The residual stream is time-major, channel-last float32 (B, T, C), compact.  bf16 exists only as an MFMA operand image (B, T + 2 * halo,
 * C) with zero halo rows around every utterance, the layout of ma_conv1d_taps_bf16.  No atomics, no cross-workgroup waiting: the same
 * bits from run to run.  All: every argument check comes before any HIP call; nothing allocates or synchronises.
 *
 * ma_mha_d128_bf16: ScaledDotProductAttention under a key-padding mask (transformer/score_function.py:21-35 as MultiHeadAttention calls
 *   it, sublayers.py:73-92), d_k in {32, 64, 128}:  ctx[b, t, h] = softmax_j(scale * q[b, t, h] . k[b, j, h], j < lens[b]) . v[b, j, h].
 *   q, k, v bf16 matrices with row strides ldq / ldk / ldv (in practice three column ranges of one fused QKV GEMM output), head h in
 *   columns h * d_k ..; utterance b starts at row b * rows_in (rows_in >= T: the operand image's T + 2 * halo).  ctx bf16, utterance b at
 *   row b * rows_out, row stride ldc.  Every one of the T query rows is computed (the reference's padded rows take part in the block's
 *   norm statistics).  Keys are walked in tiles of 32 with an online softmax; no probability reaches memory; products on MFMA, scores,
 *   running max / sum and the accumulator float32; probabilities are rounded to bf16 for the second product and the rounded values are
 *   the ones summed.  A key >= lens[b] has probability exactly 0 and neither its K nor its V row can reach the result, whatever they hold.
 *   Departure: an utterance with lens[b] <= 0 gets zero rows (the reference's softmax over all -inf gives NaN).  lens is clamped to T.
 *   Strides % 8 == 0, 16-byte aligned bases, B, H <= 65535: MA_ERR_UNSUPPORTED / MA_ERR_INVALID_ARG otherwise.
 * ma_groupnorm_stats / ma_groupnorm_apply: GroupNorm(G, C) of the (B, C, T, 1) view (sublayers.py:96-98, 141-143, with the constructor
 *   call read as 8 groups over d_model channels): per (b, group) mean and biased variance over ALL T rows x C / G channels, padded
 *   rows included.  stats: x (B, T, C) float32 -> part (B, ma_groupnorm_parts(T), G, 2) float64: mean and centred second moment of
 *   each 64-row part, fixed summation order.  apply joins the parts in part order and writes, for t < lens[b] (lens NULL: all rows),
 *   ((x - mean) * rstd) * gamma[c] + beta[c], rstd = 1 / sqrt(var + eps), and exact zeros for t >= lens[b] (the `* non_pad_mask` of
 *   layers.py:29,32): out (B, T, C) float32 (may alias x; optional) and img (B, T + 2 halo, Cpad) bf16 (optional) whose halo rows and
 *   columns C .. Cpad - 1 are written as zeros on every call.  C % G == 0, (C / G) % 4 == 0, C / 4 a divisor of 256, G <= 64, C % 8 == 0.
 * ma_fs2_layernorm_pack_f32: LayerNorm over F (biased variance, eps) of the rows t < lens[b] of x (B, T, F) float32, zeros for the other
 *   rows -> out (B, T, F) float32 (optional, may alias x) and img (B, T + 2 halo, F) bf16 with zero halo rows (optional).  The norm
 *   between the convolutions of a VariancePredictor (variance_adapter.py:74,78) and norm = "layer" of an FFT block.  F % 64 == 0, <= 1024.
 * ma_variance_head_f32: the tail of a VariancePredictor fused with its consumer (variance_adapter.py:78-89, 152-166, 305-313), one row
 *   per wave:  v = (LayerNorm_eps(hid[b, t]) . w + bias[0]) * (t < lens[b], lens NULL: 1) * control -> pred (B, T) float32;
 *   index = #{j < n_bins - 1: bins[j] < v} (searchsorted, side left) or index_in[b, t] clamped when given -> index_out (optional);
 *   x_out[b, t] = x[b, t] + table[index] as float32 (B, T, C); with pos != NULL (the decoder's position table, models.py:123) x_pos =
 *   x_out + pos[t] as float32; img (B, T + 2 halo, C) bf16 with zero halo rows holds x_pos when pos is given, x_out otherwise (each of
 *   the three optional).  table == NULL (the duration predictor): only pred is written.
 * ma_fs2_embed_f32: out[b, t] = table[ids[b, t]] + pos[t] (models.py:63-67) as float32 and as the operand image; an id outside
 *   0 .. V - 1 adds nothing.  C % 8 == 0.
 * ma_fs2_durations_f32: dur = max(round(exp(logd) - 1) * d_control, 0) (variance_adapter.py:290-291): round half to even, exp through
 *   float64 rounded once, the subtraction and the product single float32 operations (no contraction).
 * ma_length_regulate_i32: LengthRegulator on token ids (variance_adapter.py:12-31, 292).  dur (B, T_src) float32, already rounded and
 *   clipped; each is truncated to int32 (above 2^18: clamped).  -> prefix (B, T_src) exclusive sums (optional), mel_len (B), and, when
 *   expanded != NULL, expanded (B, T_cap) int32: ids[b, i] for prefix[i] <= t < prefix[i] + dur[i] by binary search, 0 (PAD) for
 *   t >= mel_len[b]; frames beyond T_cap are not written (the caller reads mel_len).  T_src <= 4096. */
int ma_mha_d128_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const int32_t* lens, int64_t B,
                     int64_t T, int64_t rows_in, int32_t H, int32_t d_k, float scale, void* ctx, int64_t ldc, int64_t rows_out,
                     ma_stream_t stream);
int32_t ma_groupnorm_parts(int64_t T);
int ma_groupnorm_stats(const float* x, int64_t B, int64_t T, int32_t C, int32_t G, double* part, ma_stream_t stream);
int ma_groupnorm_apply(const float* x, int64_t B, int64_t T, int32_t C, int32_t Cpad, int32_t G, int32_t halo, const double* part, float eps,
                       const float* gamma, const float* beta, const int32_t* lens, float* out, void* img, ma_stream_t stream);
int ma_fs2_layernorm_pack_f32(const float* x, int64_t B, int64_t T, int32_t F, int32_t halo, const float* gamma, const float* beta, float eps,
                              const int32_t* lens, float* out, void* img, ma_stream_t stream);
int ma_variance_head_f32(const float* hid, int64_t B, int64_t T, int32_t F, const float* gamma, const float* beta, float eps, const float* w,
                         const float* bias, const int32_t* lens, float control, float* pred, const float* bins, int32_t n_bins,
                         const int32_t* index_in, int32_t* index_out, const float* table, const float* x, const float* pos, int32_t C,
                         int32_t halo, float* x_out, float* x_pos, void* img, ma_stream_t stream);
int ma_fs2_embed_f32(const int32_t* ids, int64_t B, int64_t T, int32_t C, int32_t V, int32_t halo, const float* table, const float* pos,
                     float* out, void* img, ma_stream_t stream);
int ma_fs2_durations_f32(const float* logd, int64_t n, float d_control, float* dur, ma_stream_t stream);
int ma_length_regulate_i32(const float* dur, const int32_t* ids, int64_t B, int32_t T_src, int32_t* prefix, int32_t* mel_len,
                           int32_t* expanded, int32_t T_cap, ma_stream_t stream);

/* One FFT block (transformer/layers.py:27-34, sublayers.py:64-100, 130-145): device pointers.  w_qkv (3 C, C) bf16 = w_qs | w_ks | w_vs
 * stacked by rows, b_qkv [3 C]; w_fc (C, C) bf16; w_1 (d_inner, k1, C) bf16, w_2 (C, d_inner) bf16 (kernel 1); gamma / beta [C] of the
 * two norms. */
typedef struct ma_fs2_layer {
  const void* w_qkv;
  const float* b_qkv;
  const void* w_fc;
  const float* b_fc;
  const float *gamma1, *beta1;
  const void* w_1;
  const float* b_1;
  const void* w_2;
  const float* b_2;
  const float *gamma2, *beta2;
} ma_fs2_layer_t;

/* A stack of FFT blocks for one (B, T) shape: plain data.  groups > 0: GroupNorm(groups, d_model); groups == 0: LayerNorm.  halo >= k1 / 2.
 * d_model % 64 == 0 (<= 1024), d_inner % 64 == 0, d_model / heads in {32, 64, 128}. */
typedef struct ma_fs2_plan {
  int32_t n_layers, heads, d_model, d_inner, k1, groups, halo, reserved;
  int64_t B, T;
  float eps;
  int32_t reserved2;
  const ma_fs2_layer_t* layers; /* host */
} ma_fs2_plan_t;

/* ma_fs2_fft_stack: the blocks of one stack over one workspace inside one call: per block the QKV product (one N = 3 C GEMM over the
 *   operand image), ma_mha_d128_bf16, fc with the residual in its epilogue, the norm (x and img rewritten), w_1 with bias and ReLU (one
 *   ma_conv1d_taps_bf16 per utterance), w_2 with the residual in its epilogue, the norm.  x (B, T, C) float32 and img (B, T + 2 halo, C)
 *   bf16 hold the stack's input on entry and its output on return; lens (B) masks keys and rows.  No host synchronisation, read-back
 *   or allocation between the first and the last launch.  MA_ERR_WORKSPACE when workspace_bytes < ma_fs2_workspace_bytes(plan) (a
 *   negative MA_ERR_* for a plan the stack would refuse); a failed launch returns MA_ERR_LAUNCH and ends the call. */
int64_t ma_fs2_workspace_bytes(const ma_fs2_plan_t* plan);
int ma_fs2_fft_stack(const ma_fs2_plan_t* plan, float* x, void* img, const int32_t* lens, void* workspace, int64_t workspace_bytes,
                     ma_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINDAUDIO_AMD_H_ */
