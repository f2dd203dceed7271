#!/usr/bin/env python3
"""ECAPA speaker-classification head, forward + backward, at the example's shape (B, D, N) = (192, 192, 7205) and at the class count
of VoxCeleb1 alone, (192, 192, 1211): the hand-written kernels (ma_aam_softmax_fwd_f32 + ma_aam_softmax_bwd_f32, 6 launches) beside
the same formulas written in PyTorch-ROCm ops with autograd, on the same GPU, in the same process, alternating.

Prints one JSON line per shape:
  ours_us / torch_us        device events around --iters forward + backward pairs after warm-up; the median of --repeats such windows
                            (the stream's wall time: host gaps between launches included, which is what a training step pays)
  ours_spread_us / ...      smallest and largest window
  ratio_torch_over_ours     > 1: the hand-written path is faster
  launches_ours / _torch    device kernels of one forward + backward, counted by torch.profiler (null when it reports none)
  must_move_mb              W, dW, x, dx once each; output written once and read twice (from the shapes)
  hbm_floor_us              must_move over the 8 TB/s peak of the MI355X; fraction_of_hbm_floor = hbm_floor_us / ours_us
  flop_g                    2 B N D for each of the three products
  max_abs_loss_diff         |loss ours - loss torch| on the timed inputs (both float32)
No threshold: the figures are measurements."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_BYTES_PER_S = 8.0e12


def torch_head(torch, x, W, y, m, s, eps):
    e = x / torch.sqrt(torch.clamp((x * x).sum(1, keepdim=True), min=eps))
    w = W / torch.sqrt(torch.clamp((W * W).sum(1, keepdim=True), min=eps))
    c = e @ w.t()
    sine = torch.sqrt(torch.clamp(1.0 - c * c, min=0.0))
    phi = c * math.cos(m) - sine * math.sin(m)
    phi = torch.where(c > math.cos(math.pi - m), phi, c - math.sin(math.pi - m) * m)
    onehot = torch.nn.functional.one_hot(y, W.shape[0]).to(x.dtype)
    out = s * (onehot * phi + (1.0 - onehot) * c)
    loss = (torch.logsumexp(out, 1) - out.gather(1, y[:, None])[:, 0]).mean()
    correct = (out.argmax(1) == y).sum()
    return loss, correct


def must_move_bytes(b, d, n):
    return 4 * (2 * n * d + 2 * b * d + 3 * b * n)


def count_kernels(torch, fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="192x192x7205,192x192x1211")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)

    import torch

    from mindaudio_amd import _host, ops

    _host.require_gpu()
    margin, scale, eps = 0.2, 30.0, 1e-4
    for shape in a.shapes.split(","):
        b, d, n = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(0)
        x = torch.randn(b, d, generator=g).cuda()
        W = (0.1 * torch.randn(n, d, generator=g)).cuda()
        y64 = torch.randint(0, n, (b,), generator=g).cuda()
        y32 = y64.to(torch.int32)
        gs = torch.full((1,), 16384.0, device="cuda")
        dx, dw = torch.empty_like(x), torch.empty_like(W)
        xt, Wt = x.clone().requires_grad_(True), W.clone().requires_grad_(True)

        def ours():
            output, _, loss, _, saved = ops.aam_softmax_fwd(x, W, y32, margin, scale, False, eps)
            ops.aam_softmax_bwd(x, W, y32, output, saved, gs, 0.0, scale, eps, dx=dx, dw=dw)
            return loss

        def composite():
            xt.grad = Wt.grad = None
            loss, _ = torch_head(torch, xt, Wt, y64, margin, scale, eps)
            (loss * 16384.0).backward()
            return loss

        def window(fn):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.iters):
                fn()
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end) * 1e3 / a.iters

        for _ in range(a.warmup):
            ours()
            composite()
        torch.cuda.synchronize()
        t_ours, t_torch = [], []
        for _ in range(a.repeats):  # alternating: both see the same machine
            t_ours.append(window(ours))
            t_torch.append(window(composite))
        diff = abs(float(ours()) - float(composite()))
        nbytes = must_move_bytes(b, d, n)
        floor_us = nbytes / HBM_PEAK_BYTES_PER_S * 1e6
        med_ours, med_torch = statistics.median(t_ours), statistics.median(t_torch)
        print(json.dumps({
            "shape": [b, d, n], "device": torch.cuda.get_device_name(0), "iters": a.iters, "repeats": a.repeats,
            "ours_us": round(med_ours, 2), "ours_spread_us": [round(min(t_ours), 2), round(max(t_ours), 2)],
            "torch_us": round(med_torch, 2), "torch_spread_us": [round(min(t_torch), 2), round(max(t_torch), 2)],
            "ratio_torch_over_ours": round(med_torch / med_ours, 3),
            "launches_ours": count_kernels(torch, ours), "launches_torch": count_kernels(torch, composite),
            "must_move_mb": round(nbytes / 1e6, 2), "hbm_floor_us": round(floor_us, 2),
            "fraction_of_hbm_floor": round(floor_us / med_ours, 4), "flop_g": round(6.0 * b * n * d / 1e9, 3),
            "max_abs_loss_diff": diff,
        }), flush=True)


if __name__ == "__main__":
    main()
