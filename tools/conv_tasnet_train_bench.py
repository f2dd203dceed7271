#!/usr/bin/env python3
"""Conv-TasNet training step at the example's shape: the model of examples/conv_tasnet/conv_tasnet.yaml (N 512, L 20, B 256, H 512,
P 3, X 8, R 4, C 2) on 4 segments of 32000 samples (K = 3199 frames), l2 0.01, momentum from --momentum.

Prints one JSON line with
  step               median_ms / min_ms of --repeats (7) device-event timings of ConvTasNetTrainer.step (the loss read-back included)
  forward / loss / backward / update
                     the same step split by device events recorded between its phases, medians of the same repeats (the loss phase
                     holds the pairwise SI-SNR kernel, the permutation choice in torch ops and the read-back of the loss)
  launches           library launches per step, counted from the model's shape, as `total` and per phase in `detail`; bf16 mode:
                     forward 3 + 6 per block + 3, backward 5 + 11 per block (a cast, two dW products of two launches each, two dX
                     products, the launches (a), (b), (c)) + 8, update 2
  peak_memory_mb     torch.cuda.max_memory_allocated over the timed steps
  eager_f32          the same step in PyTorch-ROCm eager float32 autograd + torch.optim.SGD on the same GPU: median_ms, peak_memory_mb,
                     `speedup` = eager / step
The reference itself runs on MindSpore, which is not installed here: nothing is said about its speed.
Every timing follows warm-up steps; a repeat is one step between two device events after a synchronize.  No threshold: the figures
are measurements."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.conv_tasnet_bench import CFG, eager_forward  # noqa: E402


def eager_loss(model, x, src):
    """-mean(max over the two permutations of the mean SI-SNR), full lengths (separation_loss.py:176-250), in torch ops."""
    import torch

    est = eager_forward(model, x)
    e, t = est - est.mean(2, keepdim=True), src - src.mean(2, keepdim=True)
    e, t = e[:, :, None, :], t[:, None, :, :]
    proj = (e * t).sum(3, keepdim=True) * t / ((t ** 2).sum(3, keepdim=True) + 1e-8)
    pair = 10 * torch.log10((proj ** 2).sum(3) / (((e - proj) ** 2).sum(3) + 1e-8) + 1e-8)
    both = torch.stack([pair[:, 0, 0] + pair[:, 1, 1], pair[:, 0, 1] + pair[:, 1, 0]], dim=1) / 2
    return -both.max(dim=1).values.mean()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--samples", type=int, default=32000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--operands", default="bf16")
    ap.add_argument("--skip_eager", action="store_true")
    a = ap.parse_args(argv)

    import torch

    from mindaudio_amd import _host
    from mindaudio_amd.models import ConvTasNet, ConvTasNetTrainer

    _host.require_gpu()
    torch.manual_seed(0)
    model = ConvTasNet(**CFG).cuda()
    M, K = a.batch, model.num_frames(a.samples)
    n_out = (K + 1) * (CFG["L"] // 2)
    if n_out != a.samples:
        raise SystemExit("--samples must be a multiple of L / 2 so that the estimate has the mixture's length")
    src = 0.1 * torch.randn((M, CFG["C"], a.samples), device="cuda")
    x = src.sum(1)
    lengths = [a.samples] * M
    nblk = CFG["X"] * CFG["R"]
    bf = a.operands == "bf16"
    result = {"config": CFG, "batch": M, "samples": a.samples, "frames": K, "repeats": a.repeats, "operands": a.operands,
              "device": torch.cuda.get_device_name(0)}

    trainer = ConvTasNetTrainer(model, momentum=a.momentum, weight_decay=0.01, operands=a.operands)
    marks = {}
    inner_fwd, inner_bwd = trainer._forward, trainer._backward

    def mark(name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks[name] = ev

    def fwd(*args):
        mark("fwd0")
        inner_fwd(*args)
        mark("fwd1")

    def bwd(*args):
        mark("bwd0")
        inner_bwd(*args)
        mark("bwd1")

    trainer._forward, trainer._backward = fwd, bwd
    for _ in range(a.warmup):
        trainer.step(x, src, lengths, 1e-3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    rows = {k: [] for k in ("step", "forward", "loss", "backward", "update")}
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        mark("t0")
        trainer.step(x, src, lengths, 1e-3)
        mark("t1")
        torch.cuda.synchronize()
        el = lambda p, q: marks[p].elapsed_time(marks[q])  # noqa: E731
        for k, v in (("step", el("t0", "t1")), ("forward", el("fwd0", "fwd1")), ("loss", el("fwd1", "bwd0")), ("backward", el("bwd0", "bwd1")),
                     ("update", el("bwd1", "t1"))):
            rows[k].append(v)
    for k, v in rows.items():
        result[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}
    result["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 1e6, 1)
    per_gemm_dw = 2 if bf else 1  # a split-K product and its reduction
    detail = {"forward": 2 + 1 + nblk * (6 if bf else 5) + (3 if bf else 2),
              "loss": 1,
              "backward": 2 + (1 if bf else 0) + per_gemm_dw + 1 + nblk * ((1 if bf else 0) + 2 * per_gemm_dw + 2 + 3) +
              (1 if bf else 0) + per_gemm_dw + 1 + 2 + 1,
              "update": 2 if bf else 1}
    result["launches"] = {"total": sum(detail.values()), "detail": detail}
    trainer._forward, trainer._backward = inner_fwd, inner_bwd

    if not a.skip_eager:
        del trainer
        torch.cuda.empty_cache()
        ref = ConvTasNet(**CFG).cuda()
        opt = torch.optim.SGD(ref.parameters(), lr=1e-3, momentum=a.momentum, weight_decay=0.01)

        def eager_step():
            opt.zero_grad(set_to_none=True)
            value = eager_loss(ref, x, src)
            value.backward()
            opt.step()
            return float(value.detach())

        for _ in range(a.warmup):
            eager_step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            eager_step()
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        med = statistics.median(ms)
        result["eager_f32"] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4),
                               "peak_memory_mb": round(torch.cuda.max_memory_allocated() / 1e6, 1),
                               "speedup": round(med / result["step"]["median_ms"], 2)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
