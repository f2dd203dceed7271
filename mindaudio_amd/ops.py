"""Thin Python wrappers over the Conformer C-ABI entry points (include/mindaudio_amd.h).
Tensors are torch HIP tensors used as device buffers; all arithmetic happens in the HIP kernels."""
import ctypes

import numpy as np

from . import _host, _lib


def _epilogue(bias=None, residual=None, row_scale=None, alpha=1.0, act=_lib.ACT_NONE, out_bf16=True):
    e = _lib.GemmEpilogue()
    e.bias = bias.data_ptr() if bias is not None else None
    e.residual = residual.data_ptr() if residual is not None else None
    e.row_scale = row_scale.data_ptr() if row_scale is not None else None
    e.ldr = residual.stride(0) if residual is not None else 0
    e.alpha = float(alpha)
    e.act = int(act)
    e.out_bf16 = 1 if out_bf16 else 0
    return e


def gemm(a, w, bias=None, residual=None, row_scale=None, alpha=1.0, act=_lib.ACT_NONE, out_dtype=None, out=None):
    """out (M, N) = act(a (M, K) @ w (N, K)^T + bias) * alpha * row_scale[:, None] (+ residual).
    a, w: bf16 device tensors (K contiguous); bias/row_scale/residual float32."""
    t = _host.torch()
    lib = _lib.load()
    assert a.dtype == t.bfloat16 and w.dtype == t.bfloat16 and a.dim() == 2 and w.dim() == 2
    assert a.stride(1) == 1 and w.stride(1) == 1 and a.shape[1] == w.shape[1]
    m, k = a.shape
    n = w.shape[0]
    out_dtype = out_dtype or t.bfloat16
    if out is None:
        out = t.empty((m, n), dtype=out_dtype, device=a.device)
    assert out.dtype == out_dtype and out.stride(1) == 1 and tuple(out.shape) == (m, n)
    for x in (bias, residual, row_scale):
        assert x is None or x.dtype == t.float32
    e = _epilogue(bias, residual, row_scale, alpha, act, out_dtype == t.bfloat16)
    rc = lib.ma_gemm_bf16(_host.ptr(a), a.stride(0), _host.ptr(w), w.stride(0), _host.ptr(out), out.stride(0), m, n, k,
                          ctypes.byref(e), _host.current_stream_ptr())
    _lib.check(rc, "gemm_bf16")
    return out


def conv2d_3x3s2_pack(w):
    """Fragment-ordered packed copy of w (Cout, 3, 3, C) bf16 for conv2d_3x3s2_packed; None if the shape is not covered."""
    t = _host.torch()
    lib = _lib.load()
    assert w.dtype == t.bfloat16 and w.dim() == 4 and w.is_contiguous() and w.shape[1] == 3 and w.shape[2] == 3
    cout, c = w.shape[0], w.shape[3]
    nbytes = lib.ma_conv2d_3x3s2_packed_bytes(c, cout)
    if nbytes < 0:
        return None
    packed = t.empty((nbytes // 2,), dtype=t.bfloat16, device=w.device)
    _lib.check(lib.ma_conv2d_3x3s2_pack_bf16(_host.ptr(w), c, cout, _host.ptr(packed), _host.current_stream_ptr()),
               "conv2d_3x3s2_pack_bf16")
    return packed


def conv2d_3x3s2_packed(act, packed, bias, relu=True, out=None):
    """conv2d_3x3s2_nhwc on a packed weight: act (B, H, W, 256) bf16 NHWC -> (B, Ho, Wo, 256) bf16 (into `out` if given)."""
    t = _host.torch()
    lib = _lib.load()
    assert act.dtype == t.bfloat16 and act.is_contiguous() and bias.dtype == t.float32
    b, h, wd, c = act.shape
    cout = bias.numel()
    ho, wo = (h - 3) // 2 + 1, (wd - 3) // 2 + 1
    if out is None:
        out = t.empty((b, ho, wo, cout), dtype=t.bfloat16, device=act.device)
    assert out.shape == (b, ho, wo, cout) and out.dtype == t.bfloat16 and out.is_contiguous()
    rc = lib.ma_conv2d_3x3s2_packed_nhwc_bf16(_host.ptr(act), b, h, wd, c, _host.ptr(packed), cout, _host.ptr(bias),
                                              1 if relu else 0, _host.ptr(out), _host.current_stream_ptr())
    _lib.check(rc, "conv2d_3x3s2_packed")
    return out


def gemm_rows_pack(w):
    """Fragment-ordered packed copy of w (256, K) bf16 for gemm_rows_packed; None if the shape is not covered."""
    t = _host.torch()
    lib = _lib.load()
    assert w.dtype == t.bfloat16 and w.dim() == 2 and w.stride(1) == 1
    n, k = w.shape
    nbytes = lib.ma_gemm_rows_packed_bytes(n, k)
    if nbytes < 0 or w.stride(0) % 8:
        return None
    packed = t.empty((n, nbytes // (2 * n)), dtype=t.bfloat16, device=w.device)  # K zero-padded to a multiple of 192
    _lib.check(lib.ma_gemm_rows_pack_bf16(_host.ptr(w), w.stride(0), n, k, _host.ptr(packed), _host.current_stream_ptr()),
               "gemm_rows_pack_bf16")
    return packed


def gemm_rows_packed(a, packed, bias, alpha=1.0, out=None):
    """out (M, 256) float32 = alpha * (a (M, K) bf16 @ W^T + bias) on a packed weight (gemm_rows_pack)."""
    t = _host.torch()
    lib = _lib.load()
    assert a.dtype == t.bfloat16 and a.dim() == 2 and a.stride(1) == 1 and 0 <= packed.shape[1] - a.shape[1] < 192
    assert bias.dtype == t.float32
    m, k = a.shape
    n = packed.shape[0]
    if out is None:
        out = t.empty((m, n), dtype=t.float32, device=a.device)
    assert out.dtype == t.float32 and out.stride(1) == 1 and tuple(out.shape) == (m, n)
    rc = lib.ma_gemm_rows_packed_f32(_host.ptr(a), a.stride(0), m, k, _host.ptr(packed), n, _host.ptr(bias), float(alpha),
                                     _host.ptr(out), out.stride(0), _host.current_stream_ptr())
    _lib.check(rc, "gemm_rows_packed_f32")
    return out


def gemm_k256_pack(w):
    """Fragment-ordered packed copy of w (N, 256) bf16 for gemm_packed; None if the shape is not covered (N % 256, K != 256)."""
    t = _host.torch()
    lib = _lib.load()
    assert w.dtype == t.bfloat16 and w.dim() == 2 and w.stride(1) == 1
    n, k = w.shape
    nbytes = lib.ma_gemm_k256_packed_bytes(n, k)
    if nbytes < 0:
        return None
    packed = t.empty((n, k), dtype=t.bfloat16, device=w.device)
    _lib.check(lib.ma_gemm_k256_pack_bf16(_host.ptr(w), w.stride(0), n, k, _host.ptr(packed), _host.current_stream_ptr()),
               "gemm_k256_pack_bf16")
    return packed


def gemm_packed(a, packed, bias=None, residual=None, row_scale=None, alpha=1.0, act=_lib.ACT_NONE, out_dtype=None, out=None):
    """ops.gemm on a packed weight (gemm_k256_pack): a (M, 256) bf16, packed (N, 256)."""
    t = _host.torch()
    lib = _lib.load()
    assert a.dtype == t.bfloat16 and a.dim() == 2 and a.stride(1) == 1 and a.shape[1] == packed.shape[1]
    m, k = a.shape
    n = packed.shape[0]
    out_dtype = out_dtype or t.bfloat16
    if out is None:
        out = t.empty((m, n), dtype=out_dtype, device=a.device)
    assert out.dtype == out_dtype and out.stride(1) == 1 and tuple(out.shape) == (m, n)
    e = _epilogue(bias, residual, row_scale, alpha, act, out_dtype == t.bfloat16)
    rc = lib.ma_gemm_k256_packed_bf16(_host.ptr(a), a.stride(0), _host.ptr(packed), _host.ptr(out), out.stride(0), m, n, k,
                                      ctypes.byref(e), _host.current_stream_ptr())
    _lib.check(rc, "gemm_k256_packed_bf16")
    return out


def gemm_packed_ln(a, packed, ln_gamma, ln_beta, ln_row_scale=None, eps=1e-5, bias=None, residual=None, row_scale=None,
                   alpha=1.0, act=_lib.ACT_NONE, out=None):
    """gemm_packed (N = 256, float32 out) + the LayerNorm behind it in one launch: returns (out, bf16 LayerNorm(out) * ln_row_scale)."""
    t = _host.torch()
    lib = _lib.load()
    assert a.dtype == t.bfloat16 and a.dim() == 2 and a.stride(1) == 1 and a.shape[1] == packed.shape[1]
    m, k = a.shape
    n = packed.shape[0]
    if out is None:
        out = t.empty((m, n), dtype=t.float32, device=a.device)
    assert out.dtype == t.float32 and out.stride(1) == 1 and tuple(out.shape) == (m, n)
    ln_out = t.empty((m, n), dtype=t.bfloat16, device=a.device)
    e = _epilogue(bias, residual, row_scale, alpha, act, False)
    rc = lib.ma_gemm_k256_packed_ln_bf16(_host.ptr(a), a.stride(0), _host.ptr(packed), _host.ptr(out), out.stride(0), m, n, k,
                                         ctypes.byref(e), _host.ptr(ln_gamma), _host.ptr(ln_beta), float(eps),
                                         _opt(ln_row_scale), _host.ptr(ln_out), ln_out.stride(0), _host.current_stream_ptr())
    _lib.check(rc, "gemm_k256_packed_ln_bf16")
    return out, ln_out


def ffn_pack_weights(w1, w2):
    """Fragment-ordered packed copy of (w1 (hidden, 256), w2 (256, hidden)) bf16 for ffn_packed; redo after a weight update."""
    t = _host.torch()
    lib = _lib.load()
    assert w1.dtype == t.bfloat16 and w2.dtype == t.bfloat16 and w1.is_contiguous() and w2.is_contiguous()
    hidden, d = w1.shape
    assert tuple(w2.shape) == (d, hidden)
    nbytes = lib.ma_ffn_packed_bytes(d, hidden)
    _lib.check(min(nbytes, 0), "ffn_packed_bytes")
    packed = t.empty((nbytes // 2,), dtype=t.bfloat16, device=w1.device)
    _lib.check(lib.ma_ffn_pack_weights_bf16(_host.ptr(w1), _host.ptr(w2), d, hidden, _host.ptr(packed),
                                            _host.current_stream_ptr()), "ffn_pack_weights_bf16")
    return packed


def ffn_packed(a, packed, b1, b2, x, g1=None, be1=None, g2=None, be2=None, alpha=0.5, eps=1e-5, out_dtype=None, ln_in=None):
    """ffn / ffn_ln on packed weights (ffn_pack_weights).  g1 None: x += alpha * FFN(a) in place, returns x.
    Otherwise as ffn_ln: returns the LayerNorm output (bf16 default).  ln_in = (gamma0, beta0): a is LayerNorm(x) computed
    inside the kernel (pass a=None)."""
    t = _host.torch()
    lib = _lib.load()
    assert x.dtype == t.float32 and x.stride(1) == 1
    if ln_in is None:
        assert a.dtype == t.bfloat16 and a.stride(1) == 1 and tuple(a.shape) == tuple(x.shape)
    m, d = x.shape
    hidden = b1.numel()
    mode = 0 if g1 is None else (2 if g2 is not None else 1)
    out_dtype = out_dtype or t.bfloat16
    out = t.empty((m, d), dtype=out_dtype, device=x.device) if mode else None
    rc = lib.ma_ffn_packed_bf16(_opt(a) if ln_in is None else None, a.stride(0) if ln_in is None else 0, _host.ptr(packed),
                                _host.ptr(b1), _host.ptr(b2), _host.ptr(x), x.stride(0), m, d, hidden, float(alpha), mode,
                                _opt(g1), _opt(be1), _opt(g2), _opt(be2), float(eps), _opt(out), out.stride(0) if mode else 0,
                                1 if out_dtype == t.bfloat16 else 0, _opt(ln_in[0]) if ln_in else None,
                                _opt(ln_in[1]) if ln_in else None, _host.current_stream_ptr())
    _lib.check(rc, "ffn_packed_bf16")
    return out if mode else x


def ffn_qkv_pack(w):
    """Packed copy of a dense weight w (N, 256) bf16 for the `qkv=` tail of ffn_packed / ffn_packed_pair; None if not covered."""
    t = _host.torch()
    lib = _lib.load()
    assert w.dtype == t.bfloat16 and w.dim() == 2 and w.stride(1) == 1
    n, k = w.shape
    if k != 256 or lib.ma_ffn_qkv_packed_bytes(n) < 0:
        return None
    packed = t.empty((n * k,), dtype=t.bfloat16, device=w.device)
    _lib.check(lib.ma_ffn_qkv_pack_bf16(_host.ptr(w), w.stride(0), n, _host.ptr(packed), _host.current_stream_ptr()),
               "ffn_qkv_pack_bf16")
    return packed


def ffn_packed_qkv(a, packed, b1, b2, x, g1, be1, qkv_packed, qkv_bias, alpha=0.5, eps=1e-5, ln_in=None):
    """x += alpha FFN(a) in place, then qkv = bf16(LN(x; g1, be1) @ Wq^T + qkv_bias) on the same tile; returns qkv (M, N).
    ln_in = (gamma0, beta0): a = LayerNorm(x; gamma0, beta0) computed inside the kernel (pass a=None)."""
    t = _host.torch()
    lib = _lib.load()
    assert x.dtype == t.float32 and x.stride(1) == 1
    if ln_in is None:
        assert a.dtype == t.bfloat16 and a.stride(1) == 1
    m, d = x.shape
    n = qkv_bias.numel()
    out = t.empty((m, n), dtype=t.bfloat16, device=x.device)
    rc = lib.ma_ffn_packed_qkv_bf16(_host.ptr(a) if ln_in is None else None, a.stride(0) if ln_in is None else 0,
                                    _host.ptr(packed), _host.ptr(b1), _host.ptr(b2), _host.ptr(x),
                                    x.stride(0), m, d, b1.numel(), float(alpha), _opt(ln_in[0]) if ln_in else None,
                                    _opt(ln_in[1]) if ln_in else None, _host.ptr(g1), _host.ptr(be1), float(eps),
                                    _host.ptr(qkv_packed), _host.ptr(qkv_bias), n, _host.ptr(out), out.stride(0),
                                    _host.current_stream_ptr())
    _lib.check(rc, "ffn_packed_qkv_bf16")
    return out


def ffn_packed_pair(packed_a, b1_a, b2_a, packed_b, b1_b, b2_b, x, ln_in, ln_mid, ln_next, ln_out, alpha=0.5, eps=1e-5, qkv=None):
    """Two position-wise FFNs on the same rows in one launch (the last FFN of a Conformer block and the macaron FFN of the next):
        x1 = x + alpha FFN_A(LN(x; ln_in));   x2 = LN(x1; ln_mid);   x <- x2 + alpha FFN_B(LN(x2; ln_next))   (in place)
    returns bf16 LN(x; ln_out) — or, with qkv = (packed weight from ffn_qkv_pack, bias), bf16(LN(x; ln_out) @ Wq^T + bias).
    Each ln_* is a (gamma, beta) pair; packed_* from ffn_pack_weights."""
    t = _host.torch()
    lib = _lib.load()
    assert x.dtype == t.float32 and x.stride(1) == 1
    m, d = x.shape
    if qkv is not None:
        n = qkv[1].numel()
        out = t.empty((m, n), dtype=t.bfloat16, device=x.device)
        rc = lib.ma_ffn_packed_pair_qkv_bf16(_host.ptr(packed_a), _host.ptr(b1_a), _host.ptr(b2_a), _host.ptr(packed_b),
                                             _host.ptr(b1_b), _host.ptr(b2_b), _host.ptr(x), x.stride(0), m, d, b1_a.numel(),
                                             float(alpha), _host.ptr(ln_in[0]), _host.ptr(ln_in[1]), _host.ptr(ln_mid[0]),
                                             _host.ptr(ln_mid[1]), _host.ptr(ln_next[0]), _host.ptr(ln_next[1]),
                                             _host.ptr(ln_out[0]), _host.ptr(ln_out[1]), float(eps), _host.ptr(qkv[0]),
                                             _host.ptr(qkv[1]), n, _host.ptr(out), out.stride(0), _host.current_stream_ptr())
        _lib.check(rc, "ffn_packed_pair_qkv_bf16")
        return out
    out = t.empty((m, d), dtype=t.bfloat16, device=x.device)
    rc = lib.ma_ffn_packed_pair_bf16(_host.ptr(packed_a), _host.ptr(b1_a), _host.ptr(b2_a), _host.ptr(packed_b), _host.ptr(b1_b),
                                     _host.ptr(b2_b), _host.ptr(x), x.stride(0), m, d, b1_a.numel(), float(alpha),
                                     _host.ptr(ln_in[0]), _host.ptr(ln_in[1]), _host.ptr(ln_mid[0]), _host.ptr(ln_mid[1]),
                                     _host.ptr(ln_next[0]), _host.ptr(ln_next[1]), _host.ptr(ln_out[0]), _host.ptr(ln_out[1]),
                                     float(eps), _host.ptr(out), out.stride(0), _host.current_stream_ptr())
    _lib.check(rc, "ffn_packed_pair_bf16")
    return out


def conv2d_3x3s2_nhwc(act, w, bias=None, relu=True, out_dtype=None):
    """act (B, H, W, C) bf16 NHWC, w (Cout, 3, 3, C) bf16 -> (B, Ho, Wo, Cout)."""
    t = _host.torch()
    lib = _lib.load()
    assert act.dtype == t.bfloat16 and w.dtype == t.bfloat16 and act.is_contiguous() and w.is_contiguous()
    b, h, wd, c = act.shape
    cout = w.shape[0]
    ho, wo = (h - 3) // 2 + 1, (wd - 3) // 2 + 1
    out_dtype = out_dtype or t.bfloat16
    out = t.empty((b, ho, wo, cout), dtype=out_dtype, device=act.device)
    e = _epilogue(bias, None, None, 1.0, _lib.ACT_RELU if relu else _lib.ACT_NONE, out_dtype == t.bfloat16)
    rc = lib.ma_conv2d_3x3s2_nhwc_bf16(_host.ptr(act), b, h, wd, c, _host.ptr(w), cout, _host.ptr(out),
                                       ctypes.byref(e), _host.current_stream_ptr())
    _lib.check(rc, "conv2d_3x3s2_nhwc_bf16")
    return out


def _opt(x):
    return _host.ptr(x) if x is not None else None


def layernorm(x, gamma, beta, eps=1e-5, row_scale=None, out_dtype=None, out=None):
    """x (rows, D) float32 -> LayerNorm(x) [* row_scale[:, None]] as bf16 (default) or float32."""
    t = _host.torch()
    lib = _lib.load()
    assert x.dtype == t.float32 and x.dim() == 2 and x.stride(1) == 1
    out_dtype = out_dtype or t.bfloat16
    if out is None:
        out = t.empty(x.shape, dtype=out_dtype, device=x.device)
    rc = lib.ma_layernorm_f32(_host.ptr(x), x.stride(0), x.shape[0], x.shape[1], _host.ptr(gamma), _host.ptr(beta),
                              float(eps), _opt(row_scale), _host.ptr(out), out.stride(0),
                              1 if out_dtype == t.bfloat16 else 0, _host.current_stream_ptr())
    _lib.check(rc, "layernorm")
    return out


def layernorm2(x, g1, b1, g2, b2, eps=1e-5, out2_dtype=None):
    """In place x <- LN(x; g1, b1) (float32) and returns LN(x_new; g2, b2) as bf16 (default) or float32."""
    t = _host.torch()
    lib = _lib.load()
    assert x.dtype == t.float32 and x.dim() == 2 and x.stride(1) == 1
    out2_dtype = out2_dtype or t.bfloat16
    out2 = t.empty(x.shape, dtype=out2_dtype, device=x.device)
    rc = lib.ma_layernorm2_f32(_host.ptr(x), x.stride(0), x.shape[0], x.shape[1], _host.ptr(g1), _host.ptr(b1),
                               _host.ptr(g2), _host.ptr(b2), float(eps), _host.ptr(x), x.stride(0), _host.ptr(out2),
                               out2.stride(0), 1 if out2_dtype == t.bfloat16 else 0, _host.current_stream_ptr())
    _lib.check(rc, "layernorm2")
    return out2


def subsample_conv1(x, w, bias, cmvn_mean=None, cmvn_istd=None, out=None):
    """x (B, T, idim) float32; w (C, 3, 3), bias (C) float32 -> NHWC bf16 (B, T1, F1, C) after CMVN, conv, ReLU."""
    t = _host.torch()
    lib = _lib.load()
    assert x.dtype == t.float32 and x.dim() == 3 and w.is_contiguous()  # x: any strides (e.g. a transposed fbank output)
    b, tt, idim = x.shape
    c = w.shape[0]
    shape = (b, (tt - 3) // 2 + 1, (idim - 3) // 2 + 1, c)
    if out is None:
        out = t.empty(shape, dtype=t.bfloat16, device=x.device)
    assert out.shape == shape and out.dtype == t.bfloat16 and out.is_contiguous()
    rc = lib.ma_subsample_conv1_strided_nhwc(_host.ptr(x), x.stride(0), x.stride(1), x.stride(2), b, tt, idim, _opt(cmvn_mean),
                                             _opt(cmvn_istd), _host.ptr(w), _host.ptr(bias), c, _host.ptr(out),
                                             _host.current_stream_ptr())
    _lib.check(rc, "subsample_conv1")
    return out


def subsample_fused_pack(w1, w2, idim):
    """Packed copy of the subsampling layer's two convolution weights for subsample_fused: w1 (C, 9) float32 (conv1, as bf16
    head + tail fragments), w2 (C, 3, 3, C) bf16 (conv2, fragment order); None if (idim, C) is not covered."""
    t = _host.torch()
    lib = _lib.load()
    assert w2.dtype == t.bfloat16 and w2.dim() == 4 and w2.is_contiguous() and w2.shape[1] == 3 and w2.shape[2] == 3
    c = w2.shape[0]
    nbytes = lib.ma_subsample_fused_packed_bytes(idim, c)
    if nbytes < 0 or w2.shape[3] != c:
        return None
    assert w1.dtype == t.float32 and w1.is_contiguous() and tuple(w1.shape) == (c, 9)
    packed = t.empty((nbytes // 2,), dtype=t.bfloat16, device=w2.device)
    _lib.check(lib.ma_subsample_fused_pack_bf16(_host.ptr(w1), _host.ptr(w2), idim, c, _host.ptr(packed),
                                                _host.current_stream_ptr()), "subsample_fused_pack_bf16")
    return packed


def subsample_fused(x, packed, b1, b2, cmvn_mean=None, cmvn_istd=None, out=None):
    """CMVN + both convolutions of Conv2dSubsampling4 in one launch: x (B, T, idim) float32 (any strides) -> NHWC bf16
    (B, T2, F2, C); packed from subsample_fused_pack, b1 / b2 (C) float32."""
    t = _host.torch()
    lib = _lib.load()
    assert x.dtype == t.float32 and x.dim() == 3 and b1.dtype == t.float32 and b2.dtype == t.float32
    b, tt, idim = x.shape
    c = b1.numel()
    t1, f1 = (tt - 3) // 2 + 1, (idim - 3) // 2 + 1
    shape = (b, (t1 - 3) // 2 + 1, (f1 - 3) // 2 + 1, c)
    if out is None:
        out = t.empty(shape, dtype=t.bfloat16, device=x.device)
    assert out.shape == shape and out.dtype == t.bfloat16 and out.is_contiguous()
    rc = lib.ma_subsample_fused_bf16(_host.ptr(x), x.stride(0), x.stride(1), x.stride(2), b, tt, idim, _opt(cmvn_mean),
                                     _opt(cmvn_istd), _host.ptr(packed), _host.ptr(b1), _host.ptr(b2), c, _host.ptr(out),
                                     _host.current_stream_ptr())
    _lib.check(rc, "subsample_fused")
    return out


def relpos_attention(qkv, pos, bias_u, bias_v, mask, batch, T, heads=4, d_k=64, out=None):
    """qkv (B*T, 768) bf16; pos (T, 256) bf16; bias_u/v (heads, d_k) f32; mask (B, T) f32, (B, T, T) f32 (a per-query mask: the
    streaming configuration's chunk masks, padding folded in) or None -> ctx (B*T, 256)."""
    t = _host.torch()
    lib = _lib.load()
    assert qkv.dtype == t.bfloat16 and pos.dtype == t.bfloat16 and qkv.stride(1) == 1 and pos.stride(1) == 1
    if out is None:
        out = t.empty((batch * T, heads * d_k), dtype=t.bfloat16, device=qkv.device)
    ws_bytes = lib.ma_relpos_attention_workspace_bytes(batch, T, heads, d_k)
    ws = t.empty(ws_bytes, dtype=t.uint8, device=qkv.device)
    if mask is not None and mask.dim() == 3:
        assert tuple(mask.shape) == (batch, T, T) and mask.dtype == t.float32 and mask.is_contiguous()
        rc = lib.ma_relpos_attention_qmask_bf16(_host.ptr(qkv), qkv.stride(0), _host.ptr(pos), pos.stride(0), _host.ptr(bias_u),
                                                _host.ptr(bias_v), _host.ptr(mask), batch, T, heads, d_k, _host.ptr(out),
                                                out.stride(0), _host.ptr(ws), ws_bytes, _host.current_stream_ptr())
        _lib.check(rc, "relpos_attention_qmask")
        return out
    rc = lib.ma_relpos_attention_bf16(_host.ptr(qkv), qkv.stride(0), _host.ptr(pos), pos.stride(0), _host.ptr(bias_u),
                                      _host.ptr(bias_v), _opt(mask), batch, T, heads, d_k, _host.ptr(out),
                                      out.stride(0), _host.ptr(ws), ws_bytes, _host.current_stream_ptr())
    _lib.check(rc, "relpos_attention")
    return out


def convmodule_mid(y, dw, bn_scale, bn_shift, batch, T, out=None):
    """y (B*T, 2C) bf16 -> swish(bn(depthwise(glu(y)))) as bf16 (B*T, C)."""
    t = _host.torch()
    lib = _lib.load()
    c, ks = dw.shape
    assert y.dtype == t.bfloat16 and y.shape[1] == 2 * c and y.stride(1) == 1
    if out is None:
        out = t.empty((batch * T, c), dtype=t.bfloat16, device=y.device)
    rc = lib.ma_convmodule_mid_bf16(_host.ptr(y), y.stride(0), batch, T, c, _host.ptr(dw), ks, _host.ptr(bn_scale),
                                    _host.ptr(bn_shift), _host.ptr(out), out.stride(0), _host.current_stream_ptr())
    _lib.check(rc, "convmodule_mid")
    return out


def convmid_pw2(y, dw, bn_scale, bn_shift, pw2_packed, pw2_bias, mask_rows, x, batch, T):
    """In place x += mask * (convmodule_mid(y) @ Wp2^T + bias): conv-module middle + pointwise_conv2 + residual in one launch."""
    t = _host.torch()
    lib = _lib.load()
    c, ks = dw.shape
    assert y.dtype == t.bfloat16 and y.shape[1] == 2 * c and y.stride(1) == 1 and x.dtype == t.float32 and x.stride(1) == 1
    rc = lib.ma_convmid_pw2_bf16(_host.ptr(y), y.stride(0), batch, T, c, _host.ptr(dw), ks, _host.ptr(bn_scale),
                                 _host.ptr(bn_shift), _host.ptr(pw2_packed), _host.ptr(pw2_bias), _opt(mask_rows), _host.ptr(x),
                                 x.stride(0), _host.current_stream_ptr())
    _lib.check(rc, "convmid_pw2")
    return x


def convmodule(a, pw1_packed, pw1_bias, dw, bn_scale, bn_shift, pw2_packed, pw2_bias, mask_rows, x, batch, T):
    """In place x += mask * ConvolutionModule_after_LayerNorm(a): pointwise_conv1 + GLU + depthwise + BN + Swish + pointwise_conv2
    + residual in one launch.  a (B*T, 256) bf16 = norm_conv(x) * mask; packed weights from gemm_k256_pack."""
    t = _host.torch()
    lib = _lib.load()
    c, ks = dw.shape
    assert a.dtype == t.bfloat16 and a.shape[1] == c and a.stride(1) == 1 and x.dtype == t.float32 and x.stride(1) == 1
    rc = lib.ma_convmodule_bf16(_host.ptr(a), a.stride(0), batch, T, c, _host.ptr(pw1_packed), _host.ptr(pw1_bias), _host.ptr(dw),
                                ks, _host.ptr(bn_scale), _host.ptr(bn_shift), _host.ptr(pw2_packed), _host.ptr(pw2_bias),
                                _opt(mask_rows), _host.ptr(x), x.stride(0), _host.current_stream_ptr())
    _lib.check(rc, "convmodule")
    return x


def attn_out_convmodule(ctx, wo_packed, wo_bias, ln_gamma, ln_beta, pw1_packed, pw1_bias, dw, bn_scale, bn_shift, pw2_packed,
                        pw2_bias, mask_rows, x, batch, T, eps=1e-5, out=None):
    """out <- x' + mask * ConvModule(LN(x') * mask) with x' = x + ctx @ Wo^T + wo_bias: the attention output projection,
    norm_conv and the whole ConvolutionModule in one launch.  ctx (B*T, 256) bf16.  `out` is another buffer of x's shape (a new one
    if None), never x itself: a tile reads its neighbours' residual rows (see include/mindaudio_amd.h)."""
    t = _host.torch()
    lib = _lib.load()
    c, ks = dw.shape
    assert ctx.dtype == t.bfloat16 and ctx.shape[1] == c and ctx.stride(1) == 1 and x.dtype == t.float32 and x.stride(1) == 1
    if out is None:
        out = t.empty_like(x)
    assert out.dtype == t.float32 and out.shape == x.shape and out.stride() == x.stride()
    rc = lib.ma_attn_out_convmodule_bf16(_host.ptr(ctx), ctx.stride(0), _host.ptr(wo_packed), _host.ptr(wo_bias),
                                         _host.ptr(ln_gamma), _host.ptr(ln_beta), float(eps), batch, T, c, _host.ptr(pw1_packed),
                                         _host.ptr(pw1_bias), _host.ptr(dw), ks, _host.ptr(bn_scale), _host.ptr(bn_shift),
                                         _host.ptr(pw2_packed), _host.ptr(pw2_bias), _opt(mask_rows), _host.ptr(x), _host.ptr(out),
                                         x.stride(0), _host.current_stream_ptr())
    _lib.check(rc, "attn_out_convmodule")
    return out


def cast_bf16(x):
    """float32 device tensor -> bf16 copy (round to nearest even)."""
    t = _host.torch()
    lib = _lib.load()
    assert x.dtype == t.float32 and x.is_contiguous() and x.numel() % 4 == 0
    y = t.empty(x.shape, dtype=t.bfloat16, device=x.device)
    _lib.check(lib.ma_cast_f32_bf16(_host.ptr(x), _host.ptr(y), x.numel(), _host.current_stream_ptr()), "cast_bf16")
    return y


def ctc_loss(logits, batch, T, ys_pad, hlens, ys_lens, blank=0, zero_infinity=True):
    """logits (B*T, V) float32; ys_pad (B, Lmax) int32; hlens, ys_lens (B,) int32.
    Returns (loss scalar tensor = sum(per-utterance CTC) / B, per-utterance losses)."""
    t = _host.torch()
    lib = _lib.load()
    assert logits.dtype == t.float32 and logits.stride(1) == 1 and logits.shape[0] == batch * T
    ys_pad = ys_pad.to(t.int32).contiguous()
    hlens = hlens.to(t.int32).contiguous()
    ys_lens = ys_lens.to(t.int32).contiguous()
    per = t.empty(batch, dtype=t.float32, device=logits.device)
    lse = t.empty(batch * T, dtype=t.float32, device=logits.device)
    out = t.empty(1, dtype=t.float32, device=logits.device)
    rc = lib.ma_ctc_loss_f32(_host.ptr(logits), logits.stride(0), batch, T, logits.shape[1], _host.ptr(ys_pad),
                             ys_pad.shape[1], _host.ptr(hlens), _host.ptr(ys_lens), blank, 1 if zero_infinity else 0,
                             _host.ptr(per), _host.ptr(lse), _host.ptr(out), _host.current_stream_ptr())
    _lib.check(rc, "ctc_loss")
    return out[0], per


def ctc_greedy_search(logits, batch, T, V, mask=None, blank=0):
    """logits (B*T, ld >= V) float32 -> (best (B, T) int32 masked, best_logp (B, T) f32, hyp (B, T) int32, hyp_len (B,))."""
    t = _host.torch()
    lib = _lib.load()
    dev = logits.device
    best = t.empty((batch, T), dtype=t.int32, device=dev)
    logp = t.empty((batch, T), dtype=t.float32, device=dev)
    hyp = t.empty((batch, T), dtype=t.int32, device=dev)
    hyp_len = t.empty((batch,), dtype=t.int32, device=dev)
    rc = lib.ma_ctc_greedy_search_f32(_host.ptr(logits), logits.stride(0), batch, T, V, _opt(mask), blank, _host.ptr(best),
                                      _host.ptr(logp), _host.ptr(hyp), _host.ptr(hyp_len), _host.current_stream_ptr())
    _lib.check(rc, "ctc_greedy_search")
    return best, logp, hyp, hyp_len


def ctc_topk(logits, V, k):
    """logits (rows, ld >= V) float32 -> (topk_logp (rows, k) float32, topk_index (rows, k) int32): the k largest values of
    log_softmax(row), descending, equal values lower index first (k <= 16)."""
    t = _host.torch()
    assert logits.dtype == t.float32 and logits.dim() == 2 and logits.stride(1) == 1
    rows = logits.shape[0]
    logp = t.empty((rows, k), dtype=t.float32, device=logits.device)
    index = t.empty((rows, k), dtype=t.int32, device=logits.device)
    rc = _lib.load().ma_ctc_topk_f32(_host.ptr(logits), logits.stride(0), rows, V, k, _host.ptr(logp), _host.ptr(index),
                                     _host.current_stream_ptr())
    _lib.check(rc, "ctc_topk")
    return logp, index


def ctc_prefix_beam_search(topk_logp, topk_index, batch, T, beam, mask=None, blank=0):
    """CTC prefix beam search of a batch (utils/recognize.py:273-336): topk_logp / topk_index (batch*T, beam) from ctc_topk with
    k = beam, mask (batch*T) float32 or None -> (hyp (batch, beam, T) int32, hyp_len (batch, beam) int32, score (batch, beam)
    float64, n_hyp (batch,) int32), hypotheses best first."""
    t = _host.torch()
    assert topk_logp.dtype == t.float32 and topk_index.dtype == t.int32 and topk_logp.is_contiguous() and topk_index.is_contiguous()
    assert topk_logp.numel() == batch * T * beam and topk_index.numel() == batch * T * beam
    if mask is not None:
        assert mask.dtype == t.float32 and mask.is_contiguous() and mask.numel() == batch * T
    dev = topk_logp.device
    hyp = t.empty((batch, beam, T), dtype=t.int32, device=dev)
    hyp_len = t.empty((batch, beam), dtype=t.int32, device=dev)
    score = t.empty((batch, beam), dtype=t.float64, device=dev)
    n_hyp = t.empty((batch,), dtype=t.int32, device=dev)
    rc = _lib.load().ma_ctc_prefix_beam_search_f32(_host.ptr(topk_logp), _host.ptr(topk_index), _opt(mask), batch, T, beam, blank,
                                                   _host.ptr(hyp), _host.ptr(hyp_len), _host.ptr(score), _host.ptr(n_hyp),
                                                   _host.current_stream_ptr())
    _lib.check(rc, "ctc_prefix_beam_search")
    return hyp, hyp_len, score, n_hyp


def hyp_score(logits, V, n_utt, group, L1, tokens, lens, eos, ctc_score, ctc_weight, n_hyp=None):
    """The score loop of attention_rescoring (utils/recognize.py:393-406): logits (n_utt*group*L1, ld >= V) float32 decoder scores,
    tokens (n_utt*group, >= L1 - 1) int32, lens (n_utt*group) int32, ctc_score (n_utt*group) float64, n_hyp (n_utt) int32 or None
    -> (hyp_score (n_utt*group) float64, best_index (n_utt) int32, best_score (n_utt) float64)."""
    t = _host.torch()
    assert logits.dtype == t.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] == n_utt * group * L1
    assert tokens.dtype == t.int32 and tokens.dim() == 2 and tokens.stride(1) == 1 and tokens.shape[0] == n_utt * group
    assert lens.dtype == t.int32 and lens.is_contiguous() and ctc_score.dtype == t.float64 and ctc_score.is_contiguous()
    if n_hyp is not None:
        assert n_hyp.dtype == t.int32 and n_hyp.is_contiguous() and n_hyp.numel() == n_utt
    dev = logits.device
    ws = t.empty((n_utt * group * L1,), dtype=t.float64, device=dev)
    scores = t.empty((n_utt * group,), dtype=t.float64, device=dev)
    best = t.empty((n_utt,), dtype=t.int32, device=dev)
    best_score = t.empty((n_utt,), dtype=t.float64, device=dev)
    rc = _lib.load().ma_hyp_score_f32(_host.ptr(logits), logits.stride(0), V, n_utt, group, L1, _host.ptr(tokens), tokens.stride(0),
                                      _host.ptr(lens), _opt(n_hyp), eos, _host.ptr(ctc_score), float(ctc_weight), _host.ptr(ws),
                                      _host.ptr(scores), _host.ptr(best), _host.ptr(best_score), _host.current_stream_ptr())
    _lib.check(rc, "hyp_score")
    return scores, best, best_score


# ---- the autoregressive attention decode mode (csrc/attn_decode.hip) -------------------------------------------------------------
def decoder_self_attn_step(qkv, k_in, v_in, t, k_out, v_out, heads, scale, parent=None, ctx=None):
    """One decode step of the self-attention on a key / value cache: qkv (R, 3 d) bf16 (row r's new query | key | value), k_in / v_in
    (R, Lmax, d) bf16 with t cached positions, parent (R,) int32 or None (identity) -> ctx (R, d) bf16; k_out / v_out (R, Lmax, d)
    receive rows 0..t-1 of the parent's cache and the new key / value at row t (rows above t are not written)."""
    tt = _host.torch()
    bf = tt.bfloat16
    if qkv.dtype != bf or qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] % 3:
        raise ValueError("qkv must be a (R, 3 d) bf16 tensor with contiguous rows")
    R, d = qkv.shape[0], qkv.shape[1] // 3
    for x, what in ((k_in, "k_in"), (v_in, "v_in"), (k_out, "k_out"), (v_out, "v_out")):
        if x.dtype != bf or x.dim() != 3 or not x.is_contiguous() or x.shape[0] != R or x.shape[2] != d or x.shape[1] != k_in.shape[1]:
            raise ValueError("%s must be a contiguous (R, Lmax, d) bf16 tensor" % what)
    if parent is not None and (parent.dtype != tt.int32 or not parent.is_contiguous() or parent.numel() != R):
        raise ValueError("parent must be a contiguous (R,) int32 tensor")
    if ctx is None:
        ctx = tt.empty((R, d), dtype=bf, device=qkv.device)
    if ctx.dtype != bf or tuple(ctx.shape) != (R, d) or ctx.stride(1) != 1:
        raise ValueError("ctx must be a (R, d) bf16 tensor with contiguous rows")
    rc = _lib.load().ma_decoder_self_attn_step_bf16(_host.ptr(qkv), qkv.stride(0), _host.ptr(k_in), _host.ptr(v_in), _opt(parent), R,
                                                    k_in.shape[1], int(t), int(heads), d // int(heads) if heads else 0, d,
                                                    float(scale), _host.ptr(ctx), ctx.stride(0), _host.ptr(k_out), _host.ptr(v_out),
                                                    _host.current_stream_ptr())
    _lib.check(rc, "decoder_self_attn_step")
    return ctx


def attn_beam_step(topk_logp, topk_index, scores_in, end_in, tokens_in, length, done, eos, max_new, out=None):
    """Steps 2.2-2.6 of the attention beam search for a batch (ma_attn_beam_step_f32): topk_logp / topk_index (B*N, N) from ctc_topk
    with k = N, scores_in (B*N,) float32, end_in (B*N,) int32, tokens_in (B*N, W) int32, length / done (B,) int32 updated in place
    -> (scores_out, end_out, tokens_out, parent (B*N,) global row indices, pred (B*N,)); `out` may hand in that tuple's buffers."""
    tt = _host.torch()
    i32 = tt.int32
    if topk_logp.dtype != tt.float32 or topk_index.dtype != i32 or topk_logp.dim() != 2 or topk_logp.shape != topk_index.shape or \
            not topk_logp.is_contiguous() or not topk_index.is_contiguous():
        raise ValueError("topk_logp / topk_index must be contiguous (B*N, N) float32 / int32 tensors")
    rows, n = topk_logp.shape
    if tokens_in.dtype != i32 or tokens_in.dim() != 2 or not tokens_in.is_contiguous() or tokens_in.shape[0] != rows:
        raise ValueError("tokens_in must be a contiguous (B*N, W) int32 tensor")
    if n < 1 or rows % n or length.numel() * n != rows or done.numel() * n != rows:
        raise ValueError("%d rows are not length.numel() = %d utterances of beam %d" % (rows, length.numel(), n))
    if scores_in.dtype != tt.float32 or scores_in.numel() != rows or end_in.dtype != i32 or end_in.numel() != rows or \
            length.dtype != i32 or done.dtype != i32:
        raise ValueError("scores_in (B*N,) float32, end_in (B*N,) int32, length / done (B,) int32")
    for x in (scores_in, end_in, length, done):
        if not x.is_contiguous():
            raise ValueError("the beam state must be contiguous")
    dev, w = topk_logp.device, tokens_in.shape[1]
    if out is None:
        out = (tt.empty((rows,), dtype=tt.float32, device=dev), tt.empty((rows,), dtype=i32, device=dev),
               tt.empty((rows, w), dtype=i32, device=dev), tt.empty((rows,), dtype=i32, device=dev),
               tt.empty((rows,), dtype=i32, device=dev))
    scores_out, end_out, tokens_out, parent, pred = out
    if tuple(tokens_out.shape) != (rows, w) or tokens_out.dtype != i32 or not tokens_out.is_contiguous() or \
            scores_out.dtype != tt.float32 or scores_out.numel() != rows or any(x.dtype != i32 or x.numel() != rows
                                                                                for x in (end_out, parent, pred)):
        raise ValueError("`out` does not match the beam state")
    rc = _lib.load().ma_attn_beam_step_f32(_host.ptr(topk_logp), _host.ptr(topk_index), _host.ptr(scores_in), _host.ptr(end_in),
                                           _host.ptr(tokens_in), rows // n, n, w, int(eos), int(max_new), _host.ptr(length),
                                           _host.ptr(done), _host.ptr(scores_out), _host.ptr(end_out), _host.ptr(tokens_out),
                                           _host.ptr(parent), _host.ptr(pred), _host.current_stream_ptr())
    _lib.check(rc, "attn_beam_step")
    return out


def attn_beam_best(scores, tokens, length, beam):
    """topk_fun(scores, 1) per utterance: scores (B*N,) float32, tokens (B*N, W) int32, length (B,) int32 -> (best_hyp (B, W - 1)
    int32: the first best slot's token row without column 0, best_len (B,) int32, best_score (B,) float32)."""
    tt = _host.torch()
    if scores.dtype != tt.float32 or tokens.dtype != tt.int32 or length.dtype != tt.int32 or tokens.dim() != 2 or \
            not (scores.is_contiguous() and tokens.is_contiguous() and length.is_contiguous()):
        raise ValueError("scores (B*N,) float32, tokens (B*N, W) int32 and length (B,) int32, contiguous")
    rows, w = tokens.shape
    b = length.numel()
    if beam < 1 or rows != b * beam or scores.numel() != rows:
        raise ValueError("%d rows are not %d utterances of beam %d" % (rows, b, beam))
    dev = scores.device
    hyp = tt.empty((b, w - 1), dtype=tt.int32, device=dev)
    best_len = tt.empty((b,), dtype=tt.int32, device=dev)
    best_score = tt.empty((b,), dtype=tt.float32, device=dev)
    rc = _lib.load().ma_attn_beam_best_f32(_host.ptr(scores), _host.ptr(tokens), _host.ptr(length), b, int(beam), w, _host.ptr(hyp),
                                           _host.ptr(best_len), _host.ptr(best_score), _host.current_stream_ptr())
    _lib.check(rc, "attn_beam_best")
    return hyp, best_len, best_score


# ---- speaker verification scoring (csrc/verification.hip) ------------------------------------------------------------------------
def _check_emb(x, what):
    t = _host.torch()
    if not isinstance(x, t.Tensor) or x.dim() != 2 or x.dtype != t.float32:
        raise ValueError("%s must be a 2-D float32 tensor" % what)
    if x.shape[0] < 1:
        raise ValueError("%s has no rows" % what)
    d = x.shape[1]
    if d % 32 or not 32 <= d <= 512:
        raise ValueError("%s: embedding width %d is not a multiple of 32 up to 512" % (what, d))
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
        x = x.contiguous()
    return x


def cohort_stats(queries, cohort, k=None, block_rows=None):
    """(mean, std): float64 (E,) tensors, np.mean / np.std of the `k` largest cos(queries[e], cohort[n]) over n - the values
    np.partition(s, kth=-k)[-k:] holds (evaluate2 of the reference's speaker_verification_cosine.py).  k=None: the whole cohort.
    queries (E, D), cohort (N, D): raw float32 device tensors, D a multiple of 32 up to 512.  block_rows: query rows scored per
    pass (default: the library's 512-row recommendation)."""
    t = _host.torch()
    lib = _lib.load()
    q, c = _check_emb(queries, "queries"), _check_emb(cohort, "cohort")
    if q.shape[1] != c.shape[1]:
        raise ValueError("queries and cohort differ in width: %d, %d" % (q.shape[1], c.shape[1]))
    e, n = q.shape[0], c.shape[0]
    k = n if k is None else int(k)
    if k < 1 or k > n:
        raise ValueError("kth(=%d) out of bounds (%d)" % (-k, n))  # what np.partition raises for cohort_size > N
    nbytes = lib.ma_cohort_stats_workspace_bytes(e, n)
    if nbytes < 0:
        _lib.check(int(nbytes), "cohort_stats")
    if block_rows is not None:
        if block_rows < 1:
            raise ValueError("block_rows must be positive")
        row_bytes = (n + 3) // 4 * 16  # one query row of the score block
        nbytes += (min(int(block_rows), e) - min(e, 512)) * row_bytes
    ws = _host.workspace(nbytes, q.device)
    mean = t.empty((e,), dtype=t.float64, device=q.device)
    std = t.empty((e,), dtype=t.float64, device=q.device)
    rc = lib.ma_cohort_stats_f32(_host.ptr(q), q.stride(0), _host.ptr(c), c.stride(0), e, n, q.shape[1], k, _host.ptr(mean),
                                 _host.ptr(std), _host.ptr(ws), nbytes, _host.current_stream_ptr())
    _lib.check(rc, "cohort_stats")
    return mean, std


def trial_scores(emb, enrol_idx, test_idx, mean=None, std=None, score_norm=None):
    """float64 (T,) tensor: cos(emb[enrol_idx[t]], emb[test_idx[t]]), normalised as evaluate2 does with the per-embedding cohort
    statistics of `cohort_stats`: score_norm None / "z-norm" / "t-norm" / "s-norm"."""
    t = _host.torch()
    lib = _lib.load()
    if score_norm not in _lib.SCORE_NORMS:
        raise ValueError("unknown score_norm %r (z-norm, t-norm, s-norm or None)" % (score_norm,))
    mode = _lib.SCORE_NORMS[score_norm]
    x = _check_emb(emb, "emb")
    n = x.shape[0]
    idx = []
    for name, v in (("enrol_idx", enrol_idx), ("test_idx", test_idx)):
        v = t.as_tensor(v)
        if v.dim() != 1 or v.dtype in (t.float32, t.float64, t.bfloat16, t.float16, t.bool):
            raise ValueError("%s must be a 1-D integer list" % name)
        if v.numel() and (int(v.min()) < 0 or int(v.max()) >= n):
            raise ValueError("%s holds an index outside [0, %d)" % (name, n))
        idx.append(v.to(device=x.device, dtype=t.int32).contiguous())
    if idx[0].numel() != idx[1].numel():
        raise ValueError("enrol_idx and test_idx differ in length")
    if mode:
        if mean is None or std is None:
            raise ValueError("score_norm %r needs the cohort mean and std" % (score_norm,))
        for name, v in (("mean", mean), ("std", std)):
            if v.dtype != t.float64 or tuple(v.shape) != (n,) or v.device != x.device:
                raise ValueError("%s must be a float64 (%d,) tensor on the embeddings' device" % (name, n))
        mean, std = mean.contiguous(), std.contiguous()
    nt = idx[0].numel()
    out = t.empty((nt,), dtype=t.float64, device=x.device)
    rc = lib.ma_trial_scores_f32(_host.ptr(x), x.stride(0), n, x.shape[1], _host.ptr(idx[0]), _host.ptr(idx[1]), nt,
                                 _host.ptr(mean) if mode else None, _host.ptr(std) if mode else None, mode, _host.ptr(out),
                                 _host.current_stream_ptr())
    _lib.check(rc, "trial_scores")
    return out


def running_mean_sub(x, g_mean=None, count=0):
    """emb_mean of the reference as a column-wise scan: (y, g_mean, count) with y[n] = x[n] - g_n, g_n the running mean
    (1 - w) g_{n-1} + w x[n], w = 1 / (count + n + 1); at count 0 the incoming g_mean is ignored (g = x[0]).
    x (N, D) float32 device tensor; g_mean (D,) float64 device tensor or None; returns a new g_mean and count + N."""
    t = _host.torch()
    lib = _lib.load()
    x = _check_emb(x, "x")
    n, d = x.shape
    count = int(count)
    if count < 0:
        raise ValueError("count must not be negative")
    if g_mean is None:
        if count:
            raise ValueError("a running mean is needed when count > 0")
        g = t.zeros((d,), dtype=t.float64, device=x.device)
    else:
        if tuple(g_mean.shape) != (d,):
            raise ValueError("g_mean must have shape (%d,)" % d)
        g = g_mean.to(device=x.device, dtype=t.float64).clone().contiguous()
    nbytes = lib.ma_running_mean_sub_workspace_bytes(n, d)
    ws = t.empty((max(int(nbytes), 8) // 8,), dtype=t.float64, device=x.device)
    y = t.empty((n, d), dtype=t.float32, device=x.device)
    rc = lib.ma_running_mean_sub_f32(_host.ptr(x), x.stride(0), n, d, _host.ptr(g), count, _host.ptr(y), y.stride(0), _host.ptr(ws),
                                     nbytes, _host.current_stream_ptr())
    _lib.check(rc, "running_mean_sub")
    return y, g, count + n


def sentence_mean_norm(x):
    """InputNormalization(norm_type="sentence", std_norm=False): x (B, T, F) float32 minus its per-utterance, per-feature mean over T."""
    t = _host.torch()
    lib = _lib.load()
    if not isinstance(x, t.Tensor) or x.dim() != 3 or x.dtype != t.float32 or 0 in x.shape:
        raise ValueError("x must be a non-empty (B, T, F) float32 tensor")
    x = x.contiguous()
    out = t.empty_like(x)
    b, tt, f = x.shape
    for b0 in range(0, b, 65535):
        nb = min(65535, b - b0)
        rc = lib.ma_sentence_mean_norm_f32(_host.ptr(x[b0:]), nb, tt, f, _host.ptr(out[b0:]), _host.current_stream_ptr())
        _lib.check(rc, "sentence_mean_norm")
    return out


# ---- waveform augmentation chain (csrc/augment.hip) -------------------------------------------------------------------------------
# Device parts only: (rows, n) float32 device tensors whose rows may be strided (a slice of a wider matrix), small device arrays for
# what the host decided, and `out` (rows, n_out): columns < n hold the result, the rest zeros.  Nothing here reads a value back.
def _aug_rows(x, what="x"):
    t = _host.torch()
    if not isinstance(x, t.Tensor) or not x.is_cuda or x.dim() != 2 or x.dtype != t.float32 or 0 in x.shape:
        raise ValueError("%s must be a non-empty (rows, n) float32 device tensor" % what)
    if x.shape[0] > 65535:
        raise ValueError("%s: at most 65535 rows per call" % what)
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def _aug_out(x, out, n_out=None):
    t = _host.torch()
    if out is None:
        return t.empty((x.shape[0], x.shape[1] if n_out is None else int(n_out)), dtype=t.float32, device=x.device)
    if (not isinstance(out, t.Tensor) or out.dim() != 2 or out.dtype != t.float32 or out.device != x.device or out.shape[0] != x.shape[0]
            or out.stride(1) != 1 or (out.shape[0] > 1 and out.stride(0) < out.shape[1]) or 0 in out.shape):
        raise ValueError("out must be a (rows, n_out) float32 tensor on x's device with unit column stride")
    return out


def _ld(x):
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def _aug_f64(v, shape, device, what):
    t = _host.torch()
    v = t.as_tensor(v, dtype=t.float64).to(device).contiguous()
    if tuple(v.shape) != tuple(shape):
        raise ValueError("%s must have shape %r" % (what, tuple(shape)))
    return v


def aug_row_stats(x):
    """(rows, 4) float64 device tensor: sum |x|, sum x^2, max |x|, 0 of every row."""
    t = _host.torch()
    x = _aug_rows(x)
    stats = t.empty((x.shape[0], 4), dtype=t.float64, device=x.device)
    rc = _lib.load().ma_aug_row_stats_f32(_host.ptr(x), _ld(x), x.shape[0], x.shape[1], _host.ptr(stats), _host.current_stream_ptr())
    _lib.check(rc, "aug_row_stats")
    return stats


def aug_circular_fir(x, h, out=None):
    """y[r][i] = sum_k h[k] x[r][(i - k) mod n]; h: up to 255 float32 taps on the device."""
    t = _host.torch()
    x = _aug_rows(x)
    h = h.to(device=x.device, dtype=t.float32).contiguous()
    if h.dim() != 1 or not 1 <= h.numel() <= 255:
        raise ValueError("h must hold 1 to 255 taps")
    out = _aug_out(x, out)
    rc = _lib.load().ma_aug_circular_fir_f32(_host.ptr(x), _ld(x), x.shape[0], x.shape[1], _host.ptr(h), h.numel(), _host.ptr(out),
                                             _ld(out), out.shape[1], _host.current_stream_ptr())
    _lib.check(rc, "aug_circular_fir")
    return out


def aug_fft_conv(x, h, rot=0, stats_x=None, out=None):
    """y[r][i] = sum_k h[k] x[r][(i + rot - k) mod n] (h: K <= n float32 taps on the device); with stats_x (aug_row_stats(x)) the result
    is rescaled to x's average amplitude, as reverberate(rescale_amp="avg") does."""
    t = _host.torch()
    lib = _lib.load()
    x = _aug_rows(x)
    h = h.to(device=x.device, dtype=t.float32).contiguous()
    rows, n = x.shape
    if h.dim() != 1 or not 1 <= h.numel() <= n or not 0 <= int(rot) <= h.numel():
        raise ValueError("h must hold 1 to n taps and 0 <= rot <= len(h)")
    out = _aug_out(x, out)
    nbytes = lib.ma_aug_fft_conv_workspace_bytes(rows, n, h.numel())
    if nbytes < 0:
        _lib.check(int(nbytes), "aug_fft_conv")
    ws = _host.workspace(nbytes, x.device)
    if stats_x is not None:
        stats_x = _aug_f64(stats_x, (rows, 4), x.device, "stats_x")
    rc = lib.ma_aug_fft_conv_f32(_host.ptr(x), _ld(x), rows, n, _host.ptr(h), h.numel(), int(rot),
                                 None if stats_x is None else _host.ptr(stats_x), _host.ptr(out), _ld(out), out.shape[1], _host.ptr(ws),
                                 ws.numel(), _host.current_stream_ptr())
    _lib.check(rc, "aug_fft_conv")
    return out


def aug_babble_sum(x, speakers):
    """out[r] = x[r - 1] + ... + x[r - speakers] (rows mod the batch)."""
    t = _host.torch()
    x = _aug_rows(x)
    out = t.empty(tuple(x.shape), dtype=t.float32, device=x.device)
    rc = _lib.load().ma_aug_babble_sum_f32(_host.ptr(x), _ld(x), x.shape[0], x.shape[1], int(speakers), _host.ptr(out), _ld(out),
                                           _host.current_stream_ptr())
    _lib.check(rc, "aug_babble_sum")
    return out


def aug_mix(x, mode, stats_x, noise=None, gain=1.0, params=None, stats_noise=None, out=None):
    """out = a_r x[r] + s_r noise[row(r)] with a, s computed on the device (MA_AUG_MIX_* of the header); noise (n,) is one row for the
    batch, (rows, n) one per row."""
    t = _host.torch()
    x = _aug_rows(x)
    rows, n = x.shape
    out = _aug_out(x, out)
    stats_x = _aug_f64(stats_x, (rows, 4), x.device, "stats_x")
    ldn = 0
    if noise is not None:
        noise = noise.to(device=x.device, dtype=t.float32)
        if noise.dim() == 1:
            noise = noise.contiguous()
            if noise.numel() < n:
                raise ValueError("noise is shorter than the rows")
        else:
            noise = _aug_rows(noise, "noise")
            if noise.shape[0] != rows or noise.shape[1] < n:
                raise ValueError("noise must be (rows, >= n)")
            ldn = _ld(noise)
    if params is not None:
        params = _aug_f64(params, (rows, 4), x.device, "params")
    if stats_noise is not None:
        stats_noise = _aug_f64(stats_noise, (rows, 4), x.device, "stats_noise")
    opt = lambda v: None if v is None else _host.ptr(v)  # noqa: E731
    rc = _lib.load().ma_aug_mix_f32(_host.ptr(x), _ld(x), rows, n, opt(noise), ldn, int(mode), float(gain), opt(params),
                                    _host.ptr(stats_x), opt(stats_noise), _host.ptr(out), _ld(out), out.shape[1],
                                    _host.current_stream_ptr())
    _lib.check(rc, "aug_mix")
    return out


def aug_drop_chunks(x, intervals, fill=None, fill_off=None, noise_factor=0.0, stats=None, lens=None, out=None):
    """x with the intervals (rows, n_max, 2) int32 zeroed, or filled with 2 m u - m (u = the uniform draws in `fill`, m from the row's
    amplitude in `stats`, see the header); samples outside the intervals are copied bit for bit."""
    t = _host.torch()
    x = _aug_rows(x)
    rows, n = x.shape
    out = _aug_out(x, out)
    intervals = t.as_tensor(intervals).to(device=x.device, dtype=t.int32).contiguous()
    if intervals.dim() != 3 or intervals.shape[0] != rows or intervals.shape[2] != 2 or intervals.shape[1] > 256:
        raise ValueError("intervals must be (rows, n_max <= 256, 2)")
    n_max = intervals.shape[1]
    if fill is not None:
        fill = fill.to(device=x.device, dtype=t.float32).contiguous()
        fill_off = t.as_tensor(fill_off).to(device=x.device, dtype=t.int32).contiguous()
        if tuple(fill_off.shape) != (rows, n_max):
            raise ValueError("fill_off must be (rows, n_max)")
        stats = _aug_f64(stats, (rows, 4), x.device, "stats")
        lens = _aug_f64(lens, (rows,), x.device, "lens")
    opt = lambda v: None if v is None else _host.ptr(v)  # noqa: E731
    rc = _lib.load().ma_aug_drop_chunks_f32(_host.ptr(x), _ld(x), rows, n, _host.ptr(intervals) if n_max else None, n_max, opt(fill),
                                            opt(fill_off) if fill is not None else None, float(noise_factor),
                                            opt(stats) if fill is not None else None, opt(lens) if fill is not None else None,
                                            _host.ptr(out), _ld(out), out.shape[1], _host.current_stream_ptr())
    _lib.check(rc, "aug_drop_chunks")
    return out


# ---- ECAPA speaker-classification head (csrc/aam_softmax.hip) ---------------------------------------------------------------------
def _aam_check(emb, weight, labels=None, check_labels=True):
    """Argument checks of the head, in the order the mirrors raise: shapes / dtypes / layout (ValueError), label range (ValueError),
    width (NotImplementedError), device (MindaudioAmdError).  Returns the labels as a 1-D int32 tensor on the embeddings' device
    (None without labels)."""
    t = _host.torch()
    for name, v in (("emb", emb), ("weight", weight)):
        if not isinstance(v, t.Tensor) or v.dim() != 2 or v.dtype != t.float32:
            raise ValueError("%s must be a 2-D float32 tensor" % name)
        if not v.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    b, d = emb.shape
    n = weight.shape[0]
    if weight.shape[1] != d:
        raise ValueError("emb and weight differ in width: %d, %d" % (d, weight.shape[1]))
    if b < 1 or n < 2:
        raise ValueError("the head needs at least one row and two classes")
    if labels is not None:
        labels = t.as_tensor(labels)
        if labels.dtype not in (t.int32, t.int64, t.int16, t.uint8, t.int8) or labels.dim() != 1 or labels.shape[0] != b:
            raise ValueError("labels must be %d integers" % b)
        if check_labels and (int(labels.min()) < 0 or int(labels.max()) >= n):
            raise ValueError("labels hold a class outside [0, %d)" % n)
    if d % 32 or not 32 <= d <= 512:
        raise NotImplementedError("embedding width %d is not a multiple of 32 in [32, 512]" % d)
    _host.require_gpu()
    if not emb.is_cuda or weight.device != emb.device:
        raise ValueError("emb and weight must be tensors of one HIP device")
    return None if labels is None else labels.to(device=emb.device, dtype=t.int32).contiguous()


def _aam_workspace(b, d, n, device):
    nbytes = _lib.load().ma_aam_softmax_workspace_bytes(b, d, n)
    if nbytes < 0:
        _lib.check(int(nbytes), "aam_softmax")
    return _host.workspace(nbytes, device), int(nbytes)


def aam_softmax_fwd(emb, weight, labels, margin=0.2, scale=30.0, easy_margin=False, eps=1e-4):
    """ma_aam_softmax_fwd_f32 on checked arguments (labels: int32 on the device).  Returns (output (B, N), row_loss (B), loss (1),
    correct (1, int32), saved) with saved = (inv_x, inv_w, lse, tgrad), what aam_softmax_bwd reads again."""
    t = _host.torch()
    b, d = emb.shape
    n = weight.shape[0]
    dev = emb.device
    ws, nbytes = _aam_workspace(b, d, n, dev)
    f32 = dict(dtype=t.float32, device=dev)
    output = t.empty((b, n), **f32)
    row_loss, lse, tgrad, inv_x = (t.empty((b,), **f32) for _ in range(4))
    inv_w = t.empty((n,), **f32)
    loss = t.empty((1,), **f32)
    correct = t.empty((1,), dtype=t.int32, device=dev)
    rc = _lib.load().ma_aam_softmax_fwd_f32(_host.ptr(emb), _host.ptr(weight), _host.ptr(labels), b, d, n, float(margin), float(scale),
                                            int(bool(easy_margin)), float(eps), _host.ptr(output), _host.ptr(row_loss),
                                            _host.ptr(loss), _host.ptr(correct), _host.ptr(inv_x), _host.ptr(inv_w), _host.ptr(lse),
                                            _host.ptr(tgrad), _host.ptr(ws), nbytes, _host.current_stream_ptr())
    _lib.check(rc, "aam_softmax_fwd")
    return output, row_loss, loss, correct, (inv_x, inv_w, lse, tgrad)


def aam_softmax_bwd(emb, weight, labels, output, saved, grad_scale, l2=0.0, scale=30.0, eps=1e-4, dx=None, dw=None):
    """ma_aam_softmax_bwd_f32: (dx, dW) = grad_scale (a float32 device scalar) times d loss / d (emb, weight); dW + l2 * weight."""
    t = _host.torch()
    b, d = emb.shape
    n = weight.shape[0]
    ws, nbytes = _aam_workspace(b, d, n, emb.device)
    inv_x, inv_w, lse, tgrad = saved
    dx = t.empty_like(emb) if dx is None else dx
    dw = t.empty_like(weight) if dw is None else dw
    rc = _lib.load().ma_aam_softmax_bwd_f32(_host.ptr(emb), _host.ptr(weight), _host.ptr(labels), b, d, n, float(scale), float(eps),
                                            _host.ptr(output), _host.ptr(inv_x), _host.ptr(inv_w), _host.ptr(lse), _host.ptr(tgrad),
                                            _host.ptr(grad_scale), float(l2), _host.ptr(dx), _host.ptr(dw), _host.ptr(ws), nbytes,
                                            _host.current_stream_ptr())
    _lib.check(rc, "aam_softmax_bwd")
    return dx, dw


_aam_fn = None


def _aam_function():
    """The torch.autograd.Function around the two entry points (built on first use: torch is imported lazily in this module)."""
    global _aam_fn
    if _aam_fn is not None:
        return _aam_fn
    t = _host.torch()

    class AamSoftmaxLoss(t.autograd.Function):
        @staticmethod
        def forward(ctx, emb, weight, labels, margin, scale, easy_margin, eps):
            output, _, loss, correct, saved = aam_softmax_fwd(emb, weight, labels, margin, scale, easy_margin, eps)
            ctx.save_for_backward(emb, weight, labels, output, *saved)
            ctx.head = (scale, eps)
            correct = correct.reshape(())
            ctx.mark_non_differentiable(correct, output)
            return loss.reshape(()), correct, output

        @staticmethod
        def backward(ctx, g_loss, _g_correct, _g_output):
            emb, weight, labels, output = ctx.saved_tensors[:4]
            scale, eps = ctx.head
            gs = g_loss.detach().to(dtype=t.float32).reshape(1).contiguous()
            dx, dw = aam_softmax_bwd(emb, weight, labels, output, ctx.saved_tensors[4:], gs, 0.0, scale, eps)
            return dx, dw, None, None, None, None, None

    _aam_fn = AamSoftmaxLoss
    return _aam_fn


def aam_softmax_loss(emb, weight, labels, margin=0.2, scale=30.0, easy_margin=False, eps=1e-4, return_output=False):
    """The loss head of the ECAPA example behind the embedding: cosine Classifier (lin_blocks = 0) -> AdditiveAngularMargin ->
    softmax cross-entropy (mean) -> CorrectLabelNum on the margin-penalised output.  emb (B, D), weight (N, D) contiguous float32
    device tensors, labels (B,) integers.  Returns (loss, correct[, output]); loss.backward() fills emb.grad and weight.grad through
    ma_aam_softmax_bwd_f32.  Reading the labels' range costs a device read-back when they live on the device."""
    labels = _aam_check(emb, weight, labels)
    loss, correct, output = _aam_function().apply(emb, weight, labels, float(margin), float(scale), bool(easy_margin), float(eps))
    return (loss, correct, output) if return_output else (loss, correct)


def aam_cosine(emb, weight, eps=1e-4):
    """Classifier.construct with lin_blocks = 0: cos(emb[b], weight[n]) (B, N), both sides normalised as MindSpore's L2Normalize."""
    t = _host.torch()
    _aam_check(emb, weight)
    b, d = emb.shape
    n = weight.shape[0]
    out = t.empty((b, n), dtype=t.float32, device=emb.device)
    inv_x = t.empty((b,), dtype=t.float32, device=emb.device)
    inv_w = t.empty((n,), dtype=t.float32, device=emb.device)
    rc = _lib.load().ma_aam_cosine_f32(_host.ptr(emb), _host.ptr(weight), b, d, n, float(eps), _host.ptr(out), _host.ptr(inv_x),
                                       _host.ptr(inv_w), _host.current_stream_ptr())
    _lib.check(rc, "aam_cosine")
    return out


def aam_margin(cosine, targets, margin=0.0, scale=1.0, easy_margin=False):
    """AdditiveAngularMargin.construct: scale (targets phi + (1 - targets) cosine), elementwise on float32 device tensors."""
    t = _host.torch()
    for name, v in (("outputs", cosine), ("targets", targets)):
        if not isinstance(v, t.Tensor) or v.dtype != t.float32:
            raise ValueError("%s must be a float32 tensor" % name)
    if cosine.shape != targets.shape:
        raise ValueError("outputs and targets differ in shape")
    _host.require_gpu()
    c, tg = cosine.contiguous(), targets.to(cosine.device).contiguous()
    out = t.empty_like(c)
    rc = _lib.load().ma_aam_margin_f32(_host.ptr(c), _host.ptr(tg), c.numel(), float(margin), float(scale), int(bool(easy_margin)),
                                       _host.ptr(out), _host.current_stream_ptr())
    _lib.check(rc, "aam_margin")
    return out


def si_snr_pairwise(source, estimate, lengths):
    """(B, C, C) float64 SI-SNR in dB of estimate i against target j over the first lengths[b] samples (ma_si_snr_pairwise):
    source, estimate (B, C, T) float32 device tensors, lengths (B) integers in [1, T].  Lengths given on the host (a list, an array
    or a CPU tensor) are checked against that range; lengths that already live on the device are not read back - the kernel clamps
    them to [0, T], and an utterance of length 0 comes out as 10 log10(1e-8) = -80 dB for every pair."""
    t = _host.torch()
    for name, v in (("source", source), ("estimate", estimate)):
        if not isinstance(v, t.Tensor) or v.dtype != t.float32 or v.dim() != 3:
            raise ValueError("%s must be a (B, C, T) float32 tensor" % name)
    if source.shape != estimate.shape:
        raise ValueError("source and estimate differ in shape")
    if not estimate.is_cuda:
        raise ValueError("estimate must be a tensor on the HIP device")
    b, c, n = estimate.shape
    lens = t.as_tensor(lengths)
    if lens.shape != (b,) or lens.is_floating_point():
        raise ValueError("lengths must hold one integer per utterance")
    if not lens.is_cuda and b and (int(lens.min()) < 1 or int(lens.max()) > n):
        raise ValueError("lengths must lie in [1, T]")
    _host.require_gpu()
    est = estimate.contiguous()
    src = source.to(est.device).contiguous()
    lens = lens.to(device=est.device, dtype=t.int64).contiguous()
    out = t.empty((b, c, c), dtype=t.float64, device=est.device)
    rc = _lib.load().ma_si_snr_pairwise(_host.ptr(src), _host.ptr(est), _host.ptr(lens), b, c, n, _host.ptr(out),
                                        _host.current_stream_ptr())
    _lib.check(rc, "si_snr_pairwise")
    return out


def si_snr_pit(source, estimate, lengths):
    """SI-SNR with permutation-invariant assignment (separation_loss.py:176-250).  Returns (loss, max_snr (B, 1), reordered estimate,
    perm (B, C), pairwise (B, C, C)): the best of itertools.permutations(range(C)) per utterance (the first wins ties),
    max_snr = best sum / C, loss = -mean(max_snr), reordered[b, j] = estimate[b, perm[b, j]] with the samples at and beyond
    lengths[b] zeroed.  The pairwise table comes from the kernel; choosing among the C! sums and the gather are torch ops on
    (B, C!) and (B, C, T).  `estimate` is not modified."""
    import itertools

    t = _host.torch()
    if getattr(estimate, "ndim", 0) == 3 and estimate.shape[1] > 4:  # refused before anything reaches the device
        raise NotImplementedError("permutation-invariant SI-SNR is built for 1 to 4 sources")
    pair = si_snr_pairwise(source, estimate, lengths)
    b, c, n = estimate.shape
    dev = pair.device
    perms = t.tensor(list(itertools.permutations(range(c))), dtype=t.int64, device=dev)  # (C!, C): target j <- estimate perm[j]
    tgt = t.arange(c, device=dev)
    snr_set = pair[:, perms, tgt].sum(-1)  # (B, C!)
    # (torch.max does not promise the first index among equal values; the smallest index of the maximum does)
    best = snr_set.max(dim=1, keepdim=True).values
    idx = (snr_set == best).to(t.int64).argmax(dim=1)
    max_snr = (best / c).to(t.float32)
    perm = perms[idx]  # (B, C)
    lens = t.as_tensor(lengths).to(device=dev, dtype=t.int64)
    mask = (t.arange(n, device=dev)[None, :] < lens[:, None]).to(estimate.dtype)[:, None, :]
    reordered = t.gather(estimate.to(dev), 1, perm[:, :, None].expand(b, c, n)) * mask
    return -max_snr.mean(), max_snr, reordered, perm, pair


# ---- bidirectional LSTM layer, training (csrc/lstm.hip, csrc/lstm_train.hip) --------------------------------------------------------
class LstmTape:
    """What lstm_bidir_backward needs of a training forward: the layer's input x (T, B, Kpad) bf16 (kept by reference), the tape
    buffer of ma_lstm_bidir_train_bf16 and the shape it was written for."""

    def __init__(self, x, buf, T, B, H, dir_mask):
        self.x, self.buf, self.T, self.B, self.H, self.dir_mask = x, buf, T, B, H, dir_mask

    def views(self):
        """(act (2, T, 5, B, H) float32: the activated gates i, f, g, o and c; h (2, T, B, H) bf16: the h that was fed back)."""
        t = _host.torch()
        T, B, H = self.T, self.B, self.H
        off = int(_lib.load().ma_lstm_train_tape_h_offset(T, B, H))
        act = self.buf[:2 * T * 5 * B * H * 4].view(t.float32).view(2, T, 5, B, H)
        h = self.buf[off:off + 2 * T * B * H * 2].view(t.bfloat16).view(2, T, B, H)
        return act, h


def _lstm_check(x, layer):
    t = _host.torch()
    if not isinstance(x, t.Tensor) or x.dim() != 3 or x.dtype != t.bfloat16 or not x.is_cuda or not x.is_contiguous():
        raise ValueError("x must be a contiguous (T, B, Kpad) bf16 tensor on the HIP device")
    if x.shape[2] != layer["Kpad"]:
        raise ValueError("x has %d columns, the layer was packed for %d" % (x.shape[2], layer["Kpad"]))
    return x.shape[0], x.shape[1], layer["bias"].shape[1] // 4


def lstm_bidir_train(x, layer, dir_mask=3, chunk=None, workspace=None, out_f32=None, out_bf16=None, tape_buf=None):
    """The training forward of one bidirectional LSTM layer (ma_lstm_bidir_train_bf16): x (T, B, Kpad) bf16, layer = the operands of
    models._lstm.pack_bidir_train_layer -> (out_f32 (T, B, H), out_bf16 (T, B, H), tape: LstmTape).  out_f32 / out_bf16 have the bits
    of ma_lstm_bidir_bf16 on the same operands.
    out_f32 / out_bf16 / tape_buf: caller-owned (T, B, H) float32, (T, B, H) bf16 and uint8 buffers to write into."""
    t = _host.torch()
    T, B, H = _lstm_check(x, layer)
    _host.require_gpu()
    lib, dev = _lib.load(), x.device
    chunk = chunk or max(1, min(T, (1 << 26) // (B * 4 * H)))
    nbytes, tbytes = int(lib.ma_lstm_workspace_bytes(T, B, H, chunk)), int(lib.ma_lstm_train_tape_bytes(T, B, H))
    for v, what in ((nbytes, "lstm_workspace_bytes"), (tbytes, "lstm_train_tape_bytes")):
        if v < 0:
            _lib.check(v, what)
    if workspace is None or workspace.numel() < nbytes:
        workspace = t.empty((nbytes,), dtype=t.uint8, device=dev)
    tape = t.empty((tbytes,), dtype=t.uint8, device=dev) if tape_buf is None else tape_buf
    of = t.empty((T, B, H), dtype=t.float32, device=dev) if out_f32 is None else out_f32
    ob = t.empty((T, B, H), dtype=t.bfloat16, device=dev) if out_bf16 is None else out_bf16
    for v, dt, shape in ((tape, t.uint8, (tbytes,)), (of, t.float32, (T, B, H)), (ob, t.bfloat16, (T, B, H))):
        if v.dtype != dt or tuple(v.shape) != shape or not v.is_contiguous() or v.device != dev:
            raise ValueError("a caller-owned output must be contiguous, on x's device and of shape %s" % (shape,))
    _lib.check(lib.ma_lstm_bidir_train_bf16(_host.ptr(x), T, B, layer["Kpad"], H, _host.ptr(layer["wih"]), _host.ptr(layer["whh"]),
                                            _host.ptr(layer["bias"]), dir_mask, chunk, _host.ptr(of), _host.ptr(ob), None, _host.ptr(tape),
                                            tbytes, _host.ptr(workspace), workspace.numel(), _host.current_stream_ptr()), "lstm_bidir_train")
    return of, ob, LstmTape(x, tape, T, B, H, dir_mask)


def lstm_bidir_backward(dout, tape, layer, need_dx=True, dgates=None):
    """Backward through time of the layer whose training forward wrote `tape`: dout (T, B, H) float32 = dL/d(out_f32) ->
      dgates (2, T, B, 4H) bf16   the gradient of the pre-activation gate sums per direction (ma_lstm_bidir_bwd_bf16)
      dw_ih  (2, 4H, Kpad) f32    ma_gemm_tn_bf16_f32(dgates[dir], x); the columns past the layer's K are zero, as x's are
      db     (2, 4H) f32          its column sum: the gradient of bias_ih and of bias_hh alike
      dw_hh  (2, 4H, H) f32       the same product against the tape's h one frame earlier in the direction's walk; zero for T = 1
      dx     (T, B, Kpad) f32     sum over the directions of dgates[dir] . W_ih[dir] (ma_gemm_bf16 on layer["wih_t"]); None
                                  without need_dx.
    A direction outside the forward's dir_mask has zero gradients.  dgates: a caller-owned contiguous buffer of that shape."""
    t = _host.torch()
    T, B, H, x = tape.T, tape.B, tape.H, tape.x
    if not isinstance(dout, t.Tensor) or dout.dtype != t.float32 or tuple(dout.shape) != (T, B, H) or not dout.is_cuda:
        raise ValueError("dout must be a (T, B, H) float32 tensor on the HIP device, H that of the tape")
    dout = dout.contiguous()
    lib, dev, Kpad, g4 = _lib.load(), dout.device, layer["Kpad"], 4 * H
    s = _host.current_stream_ptr()
    dg = t.empty((2, T, B, g4), dtype=t.bfloat16, device=dev) if dgates is None else dgates
    if dg.dtype != t.bfloat16 or tuple(dg.shape) != (2, T, B, g4) or not dg.is_contiguous() or dg.device != dev:
        raise ValueError("dgates must be a contiguous (2, T, B, 4H) bf16 tensor on dout's device")
    wsb = int(lib.ma_lstm_bwd_workspace_bytes(B, H))
    if wsb < 0:
        _lib.check(wsb, "lstm_bwd_workspace_bytes")
    ws = t.empty((wsb,), dtype=t.uint8, device=dev)
    _lib.check(lib.ma_lstm_bidir_bwd_bf16(_host.ptr(dout), T, B, H, _host.ptr(tape.buf), tape.buf.numel(), _host.ptr(layer["whh_bwd"]),
                                          tape.dir_mask, _host.ptr(dg), _host.ptr(ws), wsb, s), "lstm_bidir_bwd")
    _, h = tape.views()
    dw_ih = t.zeros((2, g4, Kpad), dtype=t.float32, device=dev)
    dw_hh = t.zeros((2, g4, H), dtype=t.float32, device=dev)
    db = t.zeros((2, g4), dtype=t.float32, device=dev)
    tnb = max(int(lib.ma_gemm_tn_workspace_bytes(g4, Kpad, T * B)), int(lib.ma_gemm_tn_workspace_bytes(g4, H, max(1, (T - 1) * B))))
    tn = t.empty((tnb + 256,), dtype=t.uint8, device=dev)
    dirs = [d for d in (0, 1) if tape.dir_mask & (1 << d)]
    for d in dirs:
        _lib.check(lib.ma_gemm_tn_bf16_f32(_host.ptr(dg[d]), g4, _host.ptr(x), Kpad, _host.ptr(dw_ih[d]), Kpad, g4, Kpad, T * B, g4, 1.0, 0,
                                           _host.ptr(db[d]), _host.ptr(tn), tnb, s), "lstm dW_ih")
        if T > 1:  # forward: dgates[t] with h[t - 1]; reverse: dgates[t] with h[t + 1] - a shift of B rows either way
            a, b = (dg[d, 1:], h[d, :T - 1]) if d == 0 else (dg[d, :T - 1], h[d, 1:])
            _lib.check(lib.ma_gemm_tn_bf16_f32(_host.ptr(a), g4, _host.ptr(b), H, _host.ptr(dw_hh[d]), H, g4, H, (T - 1) * B, g4, 1.0, 0,
                                               None, _host.ptr(tn), tnb, s), "lstm dW_hh")
    dx = None
    if need_dx:
        for i, d in enumerate(dirs):
            prev, dx = dx, t.empty((T, B, Kpad), dtype=t.float32, device=dev)
            e = _epilogue(residual=prev.view(T * B, Kpad) if i else None, out_bf16=False)
            _lib.check(lib.ma_gemm_bf16(_host.ptr(dg[d]), g4, _host.ptr(layer["wih_t"][d]), g4, _host.ptr(dx), Kpad, T * B, Kpad, g4,
                                        ctypes.byref(e), s), "lstm dx")
    return dict(dgates=dg, dw_ih=dw_ih, dw_hh=dw_hh, db=db, dx=dx)


# ---- DeepSpeech2's convolution front end in training mode (csrc/deepspeech2_train.hip) ---------------------------------------------------
DS2_BN_EPS = 1e-5
DS2_BN_MOMENTUM = 0.1  # moving = 0.9 * moving + 0.1 * batch: MindSpore's BatchNorm2d(momentum=0.9)
DS2_DZ2_ROWS_BEFORE, DS2_DZ2_ROWS_EXTRA = 5, 11  # zero frequency rows of the dz2 image in front of row 0, and in all


def ds2_frontend_operands(model):
    """The training operands of MaskConv from the model's float32 parameters:
      w1t  (451, 32) float32         conv1's weight, tap-major (ma_ds2_conv1_bf16's wt)
      w2   (32, 11 * 704) bf16       conv2 as 11 time taps over 22 frequency rows x 32 channels, W[co, j, df * 32 + ci], row 21 zero
      w2t  (2, 32, 11 * 384) bf16    its transpose for the input gradient, one image per parity p of the padded input row:
                                     W_p[ci, j', k * 32 + co] = w2[co, ci, p + 2 (10 - k), 10 - j'], zero where that tap does not exist
                                     (k = 11 always, k = 0 for p = 1): 12 consecutive output rows of the dz2 image, time taps reversed."""
    t = _host.torch()
    c = model.conv
    w1, w2 = c.conv1.weight.detach().to(t.float32), c.conv2.weight.detach().to(t.float32)
    dev = w2.device
    fwd = t.zeros((32, 11, 22, 32), dtype=t.float32, device=dev)
    fwd[:, :, :21, :] = w2.permute(0, 3, 2, 1)
    rev = w2.flip(3)  # [co, ci, df, j'] with j = 10 - j'
    wt = t.zeros((2, 32, 11, 12, 32), dtype=t.float32, device=dev)
    wt[0, :, :, 0:11, :] = rev[:, :, [20 - 2 * k for k in range(11)], :].permute(1, 3, 2, 0)
    wt[1, :, :, 1:11, :] = rev[:, :, [21 - 2 * k for k in range(1, 11)], :].permute(1, 3, 2, 0)
    return dict(w1t=w1.reshape(32, 451).t().contiguous(), w2=fwd.reshape(32, 11 * 704).to(t.bfloat16).contiguous(),
                w2t=wt.reshape(2, 32, 11 * 384).to(t.bfloat16).contiguous())


class Ds2FrontendTape:
    """What ds2_frontend_backward needs of ds2_frontend_train: the input x (B, 1, F, T), the raw float32 convolution outputs y1 (T1, B,
    F1, 32) and y2 (T1 * B, F2 * 32), stats1 / stats2 (96: mean | rstd | biased variance), the operands, the BatchNorm parameters and,
    by REFERENCE, the model's act1 and xin workspaces (an inference forward of the same shape in between overwrites them).
    moving (128) = the updated moving_mean | moving_variance of bn1, then of bn2; the model's own are not touched."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def ds2_frontend_train(model, x, operands=None, mark=None):
    """Train-mode MaskConv on x (B, 1, F, T): conv1 raw -> batch statistics -> tanh(BatchNorm) as the bf16 act1 image; conv2 per output
    frequency raw -> batch statistics -> tanh(BatchNorm) as the bf16 LSTM input.  Nothing is masked.  -> (xin (T1, B, Kpad) bf16, tape).
    Launches: 4 + (F2 + 3)."""
    t = _host.require_gpu()
    lib, ck = _lib.load(), _lib.check
    dev = model.fc.module.weight.device
    if dev.type != "cuda":
        raise ValueError("the model's parameters must be on the HIP device (there is no CPU path)")
    if not isinstance(x, t.Tensor):
        x = t.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
    if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != model.n_freq:
        raise ValueError("x must be (B, 1, %d, T)" % model.n_freq)
    x = x.to(dev, t.float32).contiguous()
    P = operands if operands is not None else ds2_frontend_operands(model)
    B, _, F, T = x.shape
    ws = model._workspace(B, F, T, dev)
    T1, Fpad, act1, xin = ws["T1"], ws["Fpad"], ws["act1"], ws["xin"]
    F1, F2, lda, Kpad, rows = model.F1, model.F2, Fpad * 32, xin.shape[2], T1 * B
    bn1, bn2 = model.conv.bn1, model.conv.bn2
    f32 = t.float32
    y1 = t.empty((T1, B, F1, 32), dtype=f32, device=dev)
    y2 = t.empty((rows, F2 * 32), dtype=f32, device=dev)
    np1, np2 = int(lib.ma_ds2_conv1_raw_parts(B, T)), int(lib.ma_ds2_stats_parts(rows * F2 * 32))
    part = t.empty((max(np1, np2) * 64,), dtype=t.float64, device=dev)
    stats1, stats2 = t.empty((96,), dtype=f32, device=dev), t.empty((96,), dtype=f32, device=dev)
    moving = t.empty((128,), dtype=f32, device=dev)
    e = _epilogue(out_bf16=False)
    p = _host.ptr
    with _host.pinned_stream():
        s = _host.current_stream_ptr()
        ck(lib.ma_ds2_conv1_raw_f32(p(x), B, F, T, p(P["w1t"]), p(y1), p(part), s), "ds2_conv1_raw")
        ck(lib.ma_ds2_bn_finalize_f32(p(part), np1, rows * F1, DS2_BN_EPS, DS2_BN_MOMENTUM, p(bn1.moving_mean), p(bn1.moving_variance),
                                      p(moving[0:32]), p(moving[32:64]), p(stats1), s), "ds2_bn_finalize")
        ck(lib.ma_ds2_bn_tanh_fwd_bf16(p(y1), rows, F1 * 32, p(stats1), p(bn1.gamma), p(bn1.beta),
                                       act1.data_ptr() + (5 * B * lda + 10 * 32) * 2, lda, s), "ds2_bn_tanh_fwd")
        if mark:
            mark("fe_stage1")
        first = act1.data_ptr() + 5 * B * lda * 2
        for fo in range(F2):
            ck(lib.ma_conv1d_taps_bf16(first + 2 * fo * 32 * 2, lda, rows, 704, 11, B, p(P["w2"]), y2.data_ptr() + fo * 32 * 4, F2 * 32, 32,
                                       ctypes.byref(e), s), "ds2_conv2")
        ck(lib.ma_ds2_bn_stats_f32(p(y2), rows * F2 * 32, p(part), s), "ds2_bn_stats")
        ck(lib.ma_ds2_bn_finalize_f32(p(part), np2, rows * F2, DS2_BN_EPS, DS2_BN_MOMENTUM, p(bn2.moving_mean), p(bn2.moving_variance),
                                      p(moving[64:96]), p(moving[96:128]), p(stats2), s), "ds2_bn_finalize")
        ck(lib.ma_ds2_bn_tanh_fwd_bf16(p(y2), rows, F2 * 32, p(stats2), p(bn2.gamma), p(bn2.beta), p(xin), Kpad, s), "ds2_bn_tanh_fwd")
        if mark:
            mark("fe_stage2")
    tape = Ds2FrontendTape(x=x, y1=y1, y2=y2, stats1=stats1, stats2=stats2, moving=moving, act1=act1, xin=xin, operands=P, ws=ws,
                           gamma1=bn1.gamma, beta1=bn1.beta, gamma2=bn2.gamma, beta2=bn2.beta, B=B, F=F, T=T, T1=T1, F1=F1, F2=F2,
                           Fpad=Fpad, Kpad=Kpad)
    return xin, tape


def ds2_bn_tanh_backward(y, dout, stats, gamma, beta, out, out_ld=None):
    """The BatchNorm + tanh backward of one stage (ma_ds2_bn_tanh_bwd_f32): y (rows, cols) float32 contiguous, the raw convolution
    output; dout (rows, >= cols) float32 with its row stride; out: a float32 or bf16 tensor whose first element receives dz[0, 0], row
    stride out_ld (default: cols).  -> bsum (128) = d_beta | d_gamma | mean dn | mean dn xhat."""
    t = _host.torch()
    lib = _lib.load()
    rows, cols = y.shape
    nbytes = int(lib.ma_ds2_bn_tanh_bwd_workspace_bytes(rows, cols))
    if nbytes < 0:
        _lib.check(nbytes, "ds2_bn_tanh_bwd_workspace_bytes")
    work = t.empty((nbytes,), dtype=t.uint8, device=y.device)
    bsum = t.empty((128,), dtype=t.float32, device=y.device)
    _lib.check(lib.ma_ds2_bn_tanh_bwd_f32(_host.ptr(y), _host.ptr(dout), dout.stride(0), rows, cols, _host.ptr(stats), _host.ptr(gamma),
                                          _host.ptr(beta), _host.ptr(out), cols if out_ld is None else out_ld,
                                          1 if out.dtype == t.bfloat16 else 0, _host.ptr(bsum), None, None, _host.ptr(work), nbytes,
                                          _host.current_stream_ptr()), "ds2_bn_tanh_bwd")
    return bsum


def ds2_conv1_dw(x, dz1, frames_per_wg=0):
    """conv1's weight gradient (ma_ds2_conv1_dw_f32): x (B, 1, F, T) float32, dz1 (T1, B, F1, 32) float32 -> (32, 1, 41, 11) float32."""
    t = _host.torch()
    lib = _lib.load()
    B, _, F, T = x.shape
    parts = int(lib.ma_ds2_conv1_dw_parts(B, T, frames_per_wg))
    if parts < 0:
        _lib.check(parts, "ds2_conv1_dw_parts")
    work = t.empty((parts * 451 * 32,), dtype=t.float32, device=x.device)
    dw = t.empty((32, 1, 41, 11), dtype=t.float32, device=x.device)
    _lib.check(lib.ma_ds2_conv1_dw_f32(_host.ptr(x), B, F, T, _host.ptr(dz1), frames_per_wg, _host.ptr(dw), _host.ptr(work),
                                       work.numel() * 4, _host.current_stream_ptr()), "ds2_conv1_dw")
    return dw


def ds2_frontend_backward(dxin, tape, mark=None, keep=False):
    """The backward of ds2_frontend_train from dxin (T1, B, Kpad) float32 = d loss / d xin (feature f * 32 + c; the bf16 rounding of
    xin is passed straight through).  -> {"conv.conv1.weight" (32, 1, 41, 11), "conv.conv2.weight" (32, 32, 21, 11), "conv.bn{1,2}.gamma",
    "conv.bn{1,2}.beta" (32): float32 gradients; "stats1", "stats2": the batch statistics of the forward; "launches": per piece}.
    keep: also "dz1" (T1, B, F1, 32) float32, "dz2_image" (T1 + 10, B, (F2 + 11) * 32) bf16 and "dact1" (T1 * B, F1 * 32) float32.
      BatchNorm  one ma_ds2_bn_tanh_bwd_f32 per stage; stage 2 writes dz2 as the bf16 operand image of the two products below, with 5
                 zero frames around it and 5 / 6 zero frequency rows in front of / behind its F2 rows
      conv2 dW   per (time tap j, output frequency fo) one ma_gemm_tn_bf16_f32: dz2's 32 columns of fo against act1 shifted by j - 5
                 frames at columns 2 fo * 32 .. + 703, accumulated over fo into (11, 32, 704); row 21 of the 22 is padding and dropped
      conv2 dX   per input frequency one ma_conv1d_taps_bf16 over 12 frequency rows of the dz2 image on the transposed weights of the
                 row's parity (ds2_frontend_operands)
      conv1 dW   ma_ds2_conv1_dw_f32 on the float32 dz1."""
    t = _host.torch()
    lib, ck, p = _lib.load(), _lib.check, _host.ptr
    tp = tape
    B, T1, F1, F2, Fpad, Kpad = tp.B, tp.T1, tp.F1, tp.F2, tp.Fpad, tp.Kpad
    rows, dev, f32 = T1 * B, tp.y1.device, t.float32
    if not isinstance(dxin, t.Tensor) or dxin.dtype != f32 or tuple(dxin.shape) != (T1, B, Kpad) or dxin.device != dev:
        raise ValueError("dxin must be a (T1, B, Kpad) float32 tensor on the tape's device")
    dxin = dxin.contiguous()
    F2p = F2 + DS2_DZ2_ROWS_EXTRA
    ldz, lda = F2p * 32, Fpad * 32
    img = tp.ws.get("dz2_image")
    if img is None:
        img = tp.ws["dz2_image"] = t.zeros((T1 + 10, B, ldz), dtype=t.bfloat16, device=dev)  # only the interior is ever written
    interior = img.view(-1)[(5 * B * F2p + DS2_DZ2_ROWS_BEFORE) * 32:]
    out, launches = {}, {}
    with _host.pinned_stream():
        s = _host.current_stream_ptr()
        bs2 = ds2_bn_tanh_backward(tp.y2, dxin.view(rows, Kpad), tp.stats2, tp.gamma2, tp.beta2, interior, ldz)
        launches["batchnorm"] = 3
        if mark:
            mark("fe_bn2_bwd")
        # conv2 dW
        acc = t.empty((11, 32, 704), dtype=f32, device=dev)
        tnb = int(lib.ma_gemm_tn_workspace_bytes(32, 704, rows))
        tn = t.empty((tnb + 256,), dtype=t.uint8, device=dev)
        a0 = interior.data_ptr()
        for j in range(11):
            b0 = tp.act1.data_ptr() + j * B * lda * 2
            for fo in range(F2):
                ck(lib.ma_gemm_tn_bf16_f32(a0 + fo * 32 * 2, ldz, b0 + 2 * fo * 32 * 2, lda, acc.data_ptr() + j * 32 * 704 * 4, 704, 32, 704,
                                           rows, 32, 1.0, 1 if fo else 0, None, p(tn), tnb, s), "ds2 conv2 dW")
        launches["conv2_dw"] = 2 * 11 * F2  # (a product and the sum of its splits each)
        out["conv.conv2.weight"] = acc.view(11, 32, 22, 32)[:, :, :21, :].permute(1, 3, 2, 0).contiguous()
        if mark:
            mark("fe_conv2_dw")
        # conv2 dX
        dact1 = t.empty((rows, F1 * 32), dtype=f32, device=dev)
        e = _epilogue(out_bf16=False)
        frame0 = img.data_ptr() + 5 * B * ldz * 2
        for fi in range(F1):
            r = fi + 10
            par = r & 1
            q0 = (r - par) // 2 - 10 + DS2_DZ2_ROWS_BEFORE
            ck(lib.ma_conv1d_taps_bf16(frame0 + q0 * 32 * 2, ldz, rows, 384, 11, B, p(tp.operands["w2t"][par]),
                                       dact1.data_ptr() + fi * 32 * 4, F1 * 32, 32, ctypes.byref(e), s), "ds2 conv2 dX")
        launches["conv2_dx"] = F1
        if mark:
            mark("fe_conv2_dx")
        dz1 = t.empty((T1, B, F1, 32), dtype=f32, device=dev)
        bs1 = ds2_bn_tanh_backward(tp.y1.view(rows, F1 * 32), dact1, tp.stats1, tp.gamma1, tp.beta1, dz1)
        launches["batchnorm"] += 3
        if mark:
            mark("fe_bn1_bwd")
        out["conv.conv1.weight"] = ds2_conv1_dw(tp.x, dz1)
        launches["conv1_dw"] = 2
        if mark:
            mark("fe_conv1_dw")
    for i, bs in ((1, bs1), (2, bs2)):
        out["conv.bn%d.beta" % i], out["conv.bn%d.gamma" % i] = bs[0:32], bs[32:64]
    out.update(stats1=tp.stats1, stats2=tp.stats2, launches=launches)
    if keep:
        out.update(dz1=dz1, dz2_image=img, dact1=dact1)
    return out
