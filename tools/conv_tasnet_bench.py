#!/usr/bin/env python3
"""Conv-TasNet forward at the example's shape: the model of examples/conv_tasnet/conv_tasnet.yaml (N 512, L 20, B 256, H 512, P 3,
X 8, R 4, C 2) on 4 segments of 32000 samples (K = 3199 frames).

Prints one JSON line with
  forward                 median_ms / min_ms of --repeats device-event timings of ConvTasNet.forward (every launch and the output
                          allocation included), `launches` (3 + 6 per temporal block + 3) and `must_move_mb`: the bytes that have to
                          cross HBM with the launch pieces as they are (each activation written once and read by its consumers)
  kernels                 one launch each of the pieces at the model's shapes: median_ms, and for the elementwise ones
                          must_move_mb / gb_per_s / hbm_frac against the 8 TB/s HBM figure of bench.py --full
  eager_f32 / eager_bf16  the same network written with torch.nn.functional on (M, channels, K) tensors in PyTorch-ROCm eager, on the
                          same GPU, in float32 and under bf16 autocast: median_ms and `speedup` = eager / forward
The reference itself runs on MindSpore, which is not installed here: nothing is said about its speed.
Every timing follows warm-up calls; a repeat is one call between two device events after a synchronize.
No threshold: the figures are measurements."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0  # bench.py
CFG = dict(N=512, L=20, B=256, H=512, P=3, X=8, R=4, C=2)


def eager_forward(model, x):
    """The reference's graph (conv_tasnet.py:66-77, paired overlap) in torch.nn.functional, reading the module's parameters."""
    import torch
    import torch.nn.functional as F

    def gln(y):
        mean = y.mean(dim=(1, 2), keepdim=True)
        var = (y - mean).pow(2).mean(dim=(1, 2), keepdim=True)
        return (y - mean) / torch.sqrt(var + 1e-8)

    L, N, C = model.L, model.N, model.C
    sep = model.separator
    mw = F.relu(F.conv1d(x[:, None], model.encoder.conv1d_U.weight, stride=L // 2))
    M, _, K = mw.shape
    y = F.conv1d(gln(mw), sep.bottleneck_conv1x1.weight)
    for blk in model.blocks():
        d = blk.dilation
        t = gln(F.prelu(F.conv1d(y, blk.conv1x1.weight), blk.prelu.weight))
        t = F.conv1d(t, blk.dsconv.depthwise_conv.weight, padding=d, dilation=d, groups=t.shape[1])
        y = y + F.conv1d(gln(F.prelu(t, blk.dsconv.prelu.weight)), blk.dsconv.pointwise_conv.weight)
    mask = F.relu(F.conv1d(y, sep.mask_conv1x1.weight)).view(M, C, N, K)
    frames = F.linear((mw[:, None] * mask).transpose(2, 3), model.decoder.basis_signals.weight)  # (M, C, K, L)
    h = L // 2
    body = (frames[..., :h] + frames[..., h:]).reshape(M, C, K * h)
    return F.pad(body, (0, h))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)

    import torch

    from mindaudio_amd import _host, _lib
    from mindaudio_amd.models import ConvTasNet

    _host.require_gpu()
    torch.manual_seed(0)
    model = ConvTasNet(**CFG).cuda().eval()
    x = 0.1 * torch.randn((a.batch, a.samples), device="cuda")
    N, L, B, H, C = (CFG[k] for k in "NLBHC")
    M, K = a.batch, model.num_frames(a.samples)
    rows, nblk = M * K, CFG["X"] * CFG["R"]
    result = {"config": CFG, "batch": M, "samples": a.samples, "frames": K, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}

    def timed(fn, nbytes=None):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            torch.cuda.synchronize()
            ms.append(start.elapsed_time(end))
        med = statistics.median(ms)
        out = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4)}
        if nbytes:
            out.update(must_move_mb=round(nbytes / 1e6, 2), gb_per_s=round(nbytes / 1e9 / (med * 1e-3), 1),
                       hbm_frac=round(nbytes / 1e9 / (med * 1e-3) / HBM_PEAK_GBS, 4))
        return out

    # bytes per launch piece (f = float32 rows x channels, b = bf16)
    f = lambda c: rows * c * 4  # noqa: E731
    b = lambda c: rows * c * 2  # noqa: E731
    per_block = (f(B) + b(B)) + (b(B) + f(H)) + 2 * f(H) + 2 * f(H) + (f(H) + b(H)) + (b(H) + 2 * f(B))
    total = (M * a.samples * 4 + f(N)) + (f(N) + b(N)) + (b(N) + f(B)) + nblk * per_block + (f(B) + b(B)) + (b(B) + f(C * N)) + \
        (f(C * N) + f(N) + M * C * (K + 1) * (L // 2) * 4)
    with torch.no_grad():
        out = model(x)
        ref = eager_forward(model, x)
        rel = float((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())  # (before the piece timings reuse the buffers)
        fwd = timed(lambda: model(x))
    fwd.update(launches=3 + 6 * nblk + 3, must_move_mb=round(total / 1e6, 1),
               hbm_frac=round(total / 1e9 / (fwd["median_ms"] * 1e-3) / HBM_PEAK_GBS, 4))
    result["forward"] = fwd

    # ---- the pieces, one launch each at the model's shapes ----
    lib, s = _lib.load(), None
    ws = next(iter(model._ws.values()))
    Pp = model._prepared
    blk = Pp["blocks"][0]
    ck = _lib.check
    pn, pa, pb = ws["part_n"].data_ptr(), ws["part_a"].data_ptr(), ws["part_b"].data_ptr()
    mw, nb, xb, hb, y, z, score = (ws[k] for k in ("mw", "nb", "xb", "hb", "y", "z", "score"))
    cur, nxt = ws["x"]

    def gemm(a_, k, w, o, n, residual=None):
        e = _lib.GemmEpilogue()
        e.alpha, e.out_bf16 = 1.0, 0
        if residual is not None:
            e.residual, e.ldr = residual.data_ptr(), n
        ck(lib.ma_gemm_bf16(a_.data_ptr(), k, w.data_ptr(), k, o.data_ptr(), n, rows, n, k, ctypes.byref(e), s), "gemm")

    y0 = torch.randn((rows, H), device="cuda")  # ma_prelu_gln_stats works in place in the model: time it on a copy's worth of data
    kern = {}
    kern["encode"] = timed(lambda: ck(lib.ma_tasnet_encode_f32(x.data_ptr(), M, a.samples, a.samples, Pp["enc_t"].data_ptr(), L, N,
                                                               mw.data_ptr(), pn, s), "encode"), M * a.samples * 4 + f(N))
    kern["gln_apply_N"] = timed(lambda: ck(lib.ma_gln_apply_bf16(mw.data_ptr(), M, K, N, pn, nb.data_ptr(), s), "apply"), f(N) + b(N))
    kern["gemm_bottleneck"] = timed(lambda: gemm(nb, N, Pp["bottleneck"], cur, B))
    kern["cast_B"] = timed(lambda: ck(lib.ma_cast_f32_bf16(cur.data_ptr(), xb.data_ptr(), rows * B, s), "cast"), f(B) + b(B))
    kern["gemm_conv1x1"] = timed(lambda: gemm(xb, B, blk["c1"], y, H))
    kern["prelu_gln_stats"] = timed(lambda: ck(lib.ma_prelu_gln_stats(y0.data_ptr(), M, K, H, blk["a1"].data_ptr(), y.data_ptr(), pa, s),
                                               "prelu"), 2 * f(H))
    for d in (1, 128):
        kern["gln_dwconv_prelu_d%d" % d] = timed(
            lambda: ck(lib.ma_gln_dwconv_prelu(y.data_ptr(), M, K, H, pa, blk["dw_t"].data_ptr(), 3, d, blk["a2"].data_ptr(), z.data_ptr(),
                                               pb, s), "dwconv"), 2 * f(H))
    kern["gln_apply_H"] = timed(lambda: ck(lib.ma_gln_apply_bf16(z.data_ptr(), M, K, H, pb, hb.data_ptr(), s), "apply"), f(H) + b(H))
    kern["gemm_pointwise_residual"] = timed(lambda: gemm(hb, H, blk["pw"], nxt, B, residual=cur))
    kern["gemm_mask"] = timed(lambda: gemm(xb, B, Pp["mask"], score, C * N))
    kern["decode"] = timed(lambda: ck(lib.ma_tasnet_decode_f32(score.data_ptr(), mw.data_ptr(), M, K, C, N, Pp["basis"].data_ptr(), L, 0,
                                                               out.data_ptr(), s), "decode"), f(C * N) + f(N) + out.numel() * 4)
    result["kernels"] = kern

    # ---- the same network in PyTorch-ROCm eager ----
    with torch.no_grad():
        e32 = timed(lambda: eager_forward(model, x))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            e16 = timed(lambda: eager_forward(model, x))
    for name, e in (("eager_f32", e32), ("eager_bf16", e16)):
        e["speedup"] = round(e["median_ms"] / fwd["median_ms"], 2)
        result[name] = e
    result["relrms_vs_eager_f32"] = round(rel, 5)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
