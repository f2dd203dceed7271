"""Conv-TasNet on MI355X - mirror of mindaudio.models.conv_tasnet.ConvTasNet (conv_tasnet.py:12-77), the forward (inference and
evaluation); the training step around the same weights is models/conv_tasnet_train.py.

Activations are time-major (M * K, channels) float32.  The 1 x 1 convolutions (bottleneck, conv1x1, pointwise_conv, mask_conv1x1)
are ma_gemm_bf16 calls with float32 outputs, the block's residual added in the GEMM epilogue; the strided encoder, PReLU, global
layer norm (whole-utterance float64 statistics), the depthwise dilated convolution and the masking decoder are the kernels of
csrc/conv_tasnet.hip.  bf16 occurs only as a GEMM operand; the residual stream, `mixture_w` and everything inside PReLU / gLN / the
depthwise convolution are float32.  PyTorch layers are parameter containers (their forward() is never called), named as the
reference's cells so that checkpoint names map one to one.

Quirks of the reference that are kept, because checkpoints depend on them:
  * `mask_nonlinear` is ignored - the mask is always ReLU (conv_tasnet.py:268);
  * `norm_type` is ignored - `chose_norm` always returns the global layer norm (conv_tasnet.py:407-411), whose gamma / beta are the
    constants 1 / 0 and not parameters;
  * `overlap="paired"` (default): the reference's `overlap_and_add` multiplies by a fixed 0 / 1 matrix that adds the two halves of the
    SAME frame, out[k L/2 + j] = frame_k[j] + frame_k[j + L/2], and the model appends zeros (10 at its L = 20; L / 2 here).
    `overlap="true"` is the real overlap-add, out[k L/2 + j] += frame_k[j], for weights trained elsewhere.
Both give (M, C, (K + 1) L / 2) with K = (T - L) // (L / 2) + 1."""
import ctypes

import torch
import torch.nn as nn

from .. import _host, _lib

__all__ = ["ConvTasNet"]

_OVERLAP = {"paired": 0, "true": 1}  # MA_TASNET_OVERLAP_*


class _Encoder(nn.Module):
    def __init__(self, L, N):
        super().__init__()
        self.conv1d_U = nn.Conv1d(1, N, L, stride=L // 2, bias=False)


class _Decoder(nn.Module):
    def __init__(self, N, L):
        super().__init__()
        self.basis_signals = nn.Linear(N, L, bias=False)


class _DepthwiseSeparableConv(nn.Module):
    def __init__(self, H, B, P, dilation):
        super().__init__()
        self.depthwise_conv = nn.Conv1d(H, H, P, padding=(P - 1) * dilation // 2, dilation=dilation, groups=H, bias=False)
        self.prelu = nn.PReLU()
        self.pointwise_conv = nn.Conv1d(H, B, 1, bias=False)


class _TemporalBlock(nn.Module):
    def __init__(self, B, H, P, dilation):
        super().__init__()
        self.dilation = dilation
        self.conv1x1 = nn.Conv1d(B, H, 1, bias=False)
        self.prelu = nn.PReLU()
        self.dsconv = _DepthwiseSeparableConv(H, B, P, dilation)


class _Separator(nn.Module):
    def __init__(self, N, B, H, P, X, R, C):
        super().__init__()
        self.bottleneck_conv1x1 = nn.Conv1d(N, B, 1, bias=False)
        self.temporal_conv_net = nn.ModuleList(
            [nn.ModuleList([_TemporalBlock(B, H, P, 2 ** x) for x in range(X)]) for _ in range(R)])
        self.mask_conv1x1 = nn.Conv1d(B, C * N, 1, bias=False)


def _epilogue(residual=None, ldr=0):
    e = _lib.GemmEpilogue()
    e.alpha, e.act, e.act2, e.out_bf16 = 1.0, _lib.ACT_NONE, _lib.ACT_NONE, 0
    if residual is not None:
        e.residual, e.ldr = residual, ldr
    return e


class ConvTasNet(nn.Module):
    """ConvTasNet(N, L, B, H, P, X, R, C, norm_type="gLN", causal=False, mask_nonlinear="relu", overlap="paired"): the reference's
    arguments (conv_tasnet.py:13-40) plus `overlap`.  `norm_type` and `mask_nonlinear` are accepted and, as in the reference, have no
    effect: the norm is always gLN and the mask always ReLU.  Not built (NotImplementedError, raised before any device call):
    causal=True (the reference pads (P - 1) d on both sides and never chomps, so its residual add cannot run), P != 3, odd L, L > 64,
    N / B / H that are no multiples of 64, N > 768.

    forward(mixture (M, T) float32 on the HIP device) -> (M, C, (K + 1) L / 2) float32."""

    def __init__(self, N, L, B, H, P, X, R, C, norm_type="gLN", causal=False, mask_nonlinear="relu", overlap="paired"):
        super().__init__()
        if causal:
            raise NotImplementedError("causal Conv-TasNet is not built (the reference's causal branch cannot run either)")
        if P % 2 == 0:
            raise NotImplementedError("an even kernel size P changes the sequence length; not built")
        if P != 3:
            raise NotImplementedError("the depthwise kernel is built for P = 3")
        if N % 64 or B % 64 or H % 64 or min(N, B, H) < 64:
            raise NotImplementedError("N, B and H must be multiples of 64 (the GEMM K and the 64-lane channel layout)")
        if L % 2 or L < 2:
            raise NotImplementedError("L must be even (the hop is L / 2)")
        if L > 64 or N > 768:
            raise NotImplementedError("the decoder kernel is built for L <= 64 and N <= 768")
        if X < 1 or R < 1 or C < 1:
            raise ValueError("X, R and C must be positive")
        if overlap not in _OVERLAP:
            raise ValueError("overlap must be 'paired' or 'true'")
        self.N, self.L, self.B, self.H, self.P, self.X, self.R, self.C = N, L, B, H, P, X, R, C
        self.norm_type, self.causal, self.mask_nonlinear, self.overlap = norm_type, causal, mask_nonlinear, overlap
        self.encoder = _Encoder(L, N)
        self.separator = _Separator(N, B, H, P, X, R, C)
        self.decoder = _Decoder(N, L)
        for p in self.parameters():  # weight_init="HeUniform" of every convolution (conv_tasnet.py:97, 221, 247, 299, 366, 372)
            if p.dim() > 1:
                nn.init.kaiming_uniform_(p, a=0.0)
        self._prepared = None
        self._ws = {}
        # any load_state_dict invalidates the bf16 / transposed copies of prepare() (as EcapaTDNN does)
        self.register_load_state_dict_post_hook(lambda module, _keys: setattr(module, "_prepared", None))

    def num_frames(self, T):
        return (T - self.L) // (self.L // 2) + 1

    def blocks(self):
        return [blk for rep in self.separator.temporal_conv_net for blk in rep]

    @torch.no_grad()
    def prepare(self):
        bf, f32 = torch.bfloat16, torch.float32
        self._ws = {}

        def w1x1(conv):  # (out, in, 1) -> (out, in) bf16: the GEMM's W operand as stored
            return conv.weight.detach().squeeze(-1).to(bf).contiguous()

        sep = self.separator
        P = {"enc_t": self.encoder.conv1d_U.weight.detach().to(f32).squeeze(1).t().contiguous(),  # (L, N)
             "bottleneck": w1x1(sep.bottleneck_conv1x1), "mask": w1x1(sep.mask_conv1x1),
             "basis": self.decoder.basis_signals.weight.detach().to(f32).contiguous(), "blocks": []}  # (L, N)
        for blk in self.blocks():
            P["blocks"].append(dict(
                c1=w1x1(blk.conv1x1), a1=blk.prelu.weight.detach().to(f32).contiguous(),
                dw_t=blk.dsconv.depthwise_conv.weight.detach().to(f32).squeeze(1).t().contiguous(),  # (P, H)
                a2=blk.dsconv.prelu.weight.detach().to(f32).contiguous(), pw=w1x1(blk.dsconv.pointwise_conv), d=blk.dilation))
        self._prepared = P
        return self

    def _workspace(self, M, T, K, dev):
        key = (M, T, str(dev), int(torch.cuda.current_stream().cuda_stream))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 4:
                self._ws.clear()
            lib = _lib.load()
            rows, f32, bf = M * K, torch.float32, torch.bfloat16

            def e(cols, dtype=f32):
                return torch.empty((rows, cols), dtype=dtype, device=dev)

            def part(c):
                return torch.empty((M * lib.ma_tasnet_stat_parts(K, c) * 3,), dtype=torch.float64, device=dev)

            ws = self._ws[key] = dict(mw=e(self.N), nb=e(self.N, bf), xb=e(self.B, bf), hb=e(self.H, bf), x=(e(self.B), e(self.B)),
                                      y=e(self.H), z=e(self.H), score=e(self.C * self.N), part_n=part(self.N),
                                      part_a=part(self.H), part_b=part(self.H))
        return ws

    @torch.no_grad()
    def forward(self, mixture):
        if mixture.dim() != 2:
            raise ValueError("mixture must be (M, T)")
        M, T = mixture.shape
        if T < self.L:
            raise ValueError("mixture shorter than one encoder filter (T < L)")
        if not mixture.is_cuda:
            raise ValueError("mixture must be a tensor on the HIP device (there is no CPU path)")
        dev = mixture.device
        if self.decoder.basis_signals.weight.device != dev:
            raise ValueError("mixture and the model's parameters are on different devices")
        _host.require_gpu()
        if self._prepared is None or self._prepared["basis"].device != dev:  # (.to(another device) after a forward)
            self.prepare()
        Pp, lib = self._prepared, _lib.load()
        x_in = mixture.to(torch.float32).contiguous()  # rows T apart (a (1, T) view may report any stride(0): T is passed below)
        N, L, B, H, C = self.N, self.L, self.B, self.H, self.C
        K = self.num_frames(T)
        rows = M * K
        ws = self._workspace(M, T, K, dev)
        out = torch.empty((M, C, (K + 1) * (L // 2)), dtype=torch.float32, device=dev)
        plain = _epilogue()
        ck = _lib.check
        with _host.pinned_stream():
            s = _host.current_stream_ptr()

            def gemm(a, k, w, o, n, epi):
                ck(lib.ma_gemm_bf16(a.data_ptr(), k, w.data_ptr(), k, o.data_ptr(), n, rows, n, k, ctypes.byref(epi), s), "gemm")

            mw, nb, xb, hb, y, z = ws["mw"], ws["nb"], ws["xb"], ws["hb"], ws["y"], ws["z"]
            pn, pa, pb = ws["part_n"].data_ptr(), ws["part_a"].data_ptr(), ws["part_b"].data_ptr()
            ck(lib.ma_tasnet_encode_f32(x_in.data_ptr(), M, T, T, Pp["enc_t"].data_ptr(), L, N, mw.data_ptr(), pn, s),
               "tasnet_encode")
            ck(lib.ma_gln_apply_bf16(mw.data_ptr(), M, K, N, pn, nb.data_ptr(), s), "gln_apply")
            cur, nxt = ws["x"]
            gemm(nb, N, Pp["bottleneck"], cur, B, plain)
            for blk in Pp["blocks"]:
                ck(lib.ma_cast_f32_bf16(cur.data_ptr(), xb.data_ptr(), rows * B, s), "cast")
                gemm(xb, B, blk["c1"], y, H, plain)
                ck(lib.ma_prelu_gln_stats(y.data_ptr(), M, K, H, blk["a1"].data_ptr(), y.data_ptr(), pa, s), "prelu_gln_stats")
                ck(lib.ma_gln_dwconv_prelu(y.data_ptr(), M, K, H, pa, blk["dw_t"].data_ptr(), self.P, blk["d"], blk["a2"].data_ptr(),
                                           z.data_ptr(), pb, s), "gln_dwconv_prelu")
                ck(lib.ma_gln_apply_bf16(z.data_ptr(), M, K, H, pb, hb.data_ptr(), s), "gln_apply")
                gemm(hb, H, blk["pw"], nxt, B, _epilogue(cur.data_ptr(), B))  # x + pointwise(...): two buffers, never in place
                cur, nxt = nxt, cur
            ck(lib.ma_cast_f32_bf16(cur.data_ptr(), xb.data_ptr(), rows * B, s), "cast")
            gemm(xb, B, Pp["mask"], ws["score"], C * N, plain)
            ck(lib.ma_tasnet_decode_f32(ws["score"].data_ptr(), mw.data_ptr(), M, K, C, N, Pp["basis"].data_ptr(), L,
                                        _OVERLAP[self.overlap], out.data_ptr(), s), "tasnet_decode")
        return out
