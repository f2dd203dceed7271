#!/usr/bin/env python3
"""WaveGrad training at the example's shape: examples/wavegrad/wavegrad_base.yaml, crop_mel_frames = 30 (T = 9000 samples per
utterance), random weights and data, one batch repeated.

--part ours        prints one JSON line for --batch utterances (32 = the yaml's 256 over 8 devices); medians (with min / max) of
                   --repeats steps after --warmup steps, device events:
    step           WaveGradTrainer.step (host encoding table, uploads and the read-back of loss / overflow included), wall clock
    forward        the retaining forward (ma_wavegrad_forward on the all-buffers-kept plan)
    backward       the gradient zero fill and the reverse walk
    update         norm partials, clipped Adam, the bf16 weight copies
    launches       kernel launches per phase as the trainer counts them (the products run once per utterance in the forward and in dX,
                   so the count grows with the batch)
    peak_mem_mb    torch.cuda.max_memory_allocated over a step; workspace_mb = activations + gradients of the plan; params
--part eager_f32   the same step in PyTorch-ROCm eager float32 autograd on the same GPU (tools/wavegrad_bench.py's throw-away module,
                   L1 loss, clip_grad_norm_, torch.optim.Adam): {median_ms, ...} and its peak memory, or {"error": ...}.
Each part is a process of its own so that a job script can give each its own time limit.  The reference itself runs on MindSpore, which
is not installed here: nothing is said about its speed.  No threshold: the figures are measurements."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import wavegrad_bench as WB  # noqa: E402


def batch(torch, B, frames):
    T = WB.YAML["hop_samples"] * frames
    audio, noise = torch.randn((B, T), device="cuda"), torch.randn((B, T), device="cuda")
    return audio, 0.1 + 0.8 * torch.rand((B,)), noise, torch.rand((B, WB.YAML["n_mels"], frames), device="cuda")


def ours(a, torch):
    from mindaudio_amd import _host
    from mindaudio_amd.models import WaveGrad, WaveGradTrainer

    _host.require_gpu()
    model = WaveGrad(WB.YAML).cuda()
    tr = WaveGradTrainer(model, 2e-4, max_grad_norm=1.0, operands=a.operands)
    data = batch(torch, a.batch, a.frames)
    torch.cuda.reset_peak_memory_stats()
    out = {"step": WB.timed(torch, lambda: tr.step(*data), a.warmup, a.repeats, WB._wall_ms)}
    out["peak_mem_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    out["launches"] = dict(tr.launches)
    st = tr._steps[(a.batch, a.frames)]
    out["workspace_mb"] = round((st.ws.numel() + st.gws.numel() + st.gimg.numel()) / 2 ** 20, 1)
    out["params"] = tr.params.size

    def phase(fn):
        def run():
            with torch.no_grad(), _host.pinned_stream():
                fn(_host.current_stream_ptr())
        return WB.timed(torch, run, 1, a.repeats)

    def backward(s):
        tr.params.grad.zero_()
        tr._backward(st, s)

    def update(s):  # (loss scale 2^30: the norm is tiny, the factor 1, the step a real one on whatever the gradient buffer holds)
        from mindaudio_amd import _lib

        lib, fp = _lib.load(), tr.params
        _lib.check(lib.ma_wavegrad_sumsq_f64(fp.grad.data_ptr(), fp.size, tr._norm_part.data_ptr(), s), "sumsq")
        _lib.check(lib.ma_wavegrad_clip_adam_f32(fp.master.data_ptr(), fp.grad.data_ptr(), fp.moment1.data_ptr(), fp.moment2.data_ptr(), fp.size,
                                                 tr._norm_part.data_ptr(), tr._norm_parts, tr.scaler.scale, 1.0, 2e-4, 0.9, 0.999, 1e-8,
                                                 tr._flag.data_ptr(), tr._norm.data_ptr(), s), "clip_adam")
        tr._refresh(s)

    out["forward"] = phase(lambda s: tr._forward(st, s))
    out["backward"] = phase(backward)
    out["update"] = phase(update)
    return out


def eager(a, torch):
    net = WB.eager_net(torch).cuda().train()
    opt = torch.optim.Adam(net.parameters(), lr=2e-4)
    audio, level, noise, spec = batch(torch, a.batch, a.frames)
    level = level.cuda()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = (net(audio, level, spec) - noise).abs().mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
        return float(loss.detach())

    try:
        torch.cuda.reset_peak_memory_stats()
        out = WB.timed(torch, step, a.warmup, a.repeats, WB._wall_ms)
        out["peak_mem_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        return out
    except RuntimeError as err:  # e.g. MIOpen refusing a shape: reported as it is
        return {"error": str(err).split("\n")[0][:300]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("ours", "eager_f32"), default="ours")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--operands", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("wavegrad_train_bench needs a HIP device: nothing is measured without one")
    torch.manual_seed(0)
    result = {"part": a.part, "batch": a.batch, "frames": a.frames, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    result.update(ours(a, torch) if a.part == "ours" else {"eager_f32_step": eager(a, torch)})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
