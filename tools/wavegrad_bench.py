#!/usr/bin/env python3
"""WaveGrad at the example's shape: examples/wavegrad/wavegrad_base.yaml on B = 1 utterance of --frames mel frames (300 = 4.1 s at
22.05 kHz), random weights.

--part ours        prints one JSON line; medians (with min / max) of --repeats runs after --warmup runs
    forward        one network evaluation (WaveGrad.forward: the host encoding table and the mel transpose included), device events
    loop_numpy     the --steps-step reverse loop under noise="numpy" (the reference's host draws, uploaded in chunks), wall clock
    loop_device    the same under noise="device" (torch.randn on the device), wall clock
    step_us        loop_device / steps
    launches_per_step, rtf_* = audio seconds / loop seconds, peak_mem_mb (torch.cuda.max_memory_allocated over a loop), workspace_mb
    launch_gap_us  the mean time per launch of 2000 back-to-back launches of a near-empty kernel
--part eager_f32   the same network as a throw-away module of torch.nn.functional.conv1d calls in PyTorch-ROCm eager, float32, on the
                   same GPU: one evaluation, {median_ms, ...}, or {"error": ...} if the library refuses a shape.
Each part is a process of its own so that a job script can give each its own time limit.  The reference itself runs on MindSpore, which
is not installed here: nothing is said about its speed.  No threshold: the figures are measurements."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

YAML = dict(n_mels=128, hop_samples=300, sample_rate=22050, n_fft=2048, noise_schedule_start=1e-6, noise_schedule_end=0.01,
            noise_schedule_S=1000,
            dblock=dict(init_conv_channels=32, init_conv_kernels=5, hidden_size=[128, 128, 256, 512], factor=[2, 2, 3, 5],
                        kernel_size=[3, 3, 3], dilations=[1, 2, 4]),
            film=dict(output_size=[128, 128, 256, 512, 512], kernel_size=[3, 3, 3, 3, 3]),
            ublock=dict(hidden_size=[512, 512, 256, 128, 128], factor=[5, 5, 3, 2, 2],
                        dilation=[[1, 2, 1, 2], [1, 2, 1, 2], [1, 2, 4, 8], [1, 2, 4, 8], [1, 2, 4, 8]], kernel_size=3),
            first_conv=dict(hidden_size=768, kernel_size=3), last_conv=dict(kernel_size=3))


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _event_ms(torch, fn):
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def _wall_ms(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(torch, fn, warmup, repeats, clock=_event_ms):
    for _ in range(warmup):
        fn()
    return _stats([clock(torch, fn) for _ in range(repeats)])


def ours(a, torch):
    import numpy as np

    from mindaudio_amd import _host, _lib
    from mindaudio_amd.models import WaveGrad
    from mindaudio_amd.wavegrad.reverse import reverse

    _host.require_gpu()
    lib = _lib.load()
    model = WaveGrad(YAML).cuda().eval()
    T = 300 * a.frames
    audio = torch.randn((1, T), device="cuda")
    spec = torch.rand((1, 128, a.frames), device="cuda")
    level = torch.tensor([0.5])
    out = {"launches_per_step": model.launches_per_step(1, a.frames)}
    out["workspace_mb"] = round(next(iter(model._plans.values())).ws_bytes / 2 ** 20, 1)
    out["forward"] = timed(torch, lambda: model(audio, level, spec), a.warmup, a.repeats)
    beta = np.linspace(YAML["noise_schedule_start"], YAML["noise_schedule_end"], a.steps)
    torch.cuda.reset_peak_memory_stats()
    for mode in ("numpy", "device"):
        out["loop_" + mode] = timed(torch, lambda mode=mode: reverse(model, spec, beta=beta, noise=mode, seed=1), 1, a.repeats, _wall_ms)
        out["rtf_" + mode] = round((T / YAML["sample_rate"]) / (out["loop_" + mode]["median_ms"] / 1e3), 3)
    out["peak_mem_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    out["step_us"] = round(out["loop_device"]["median_ms"] * 1e3 / a.steps, 2)
    sink = torch.zeros((1 << 16,), device="cuda")
    n = 2000

    def launches():
        for _ in range(n):
            lib.ma_valu_issue_probe(1, 1, sink.data_ptr(), None)

    gap = timed(torch, launches, 1, 5)
    out["launch_gap_us"] = round(gap["median_ms"] * 1e3 / n, 3)
    return out


def eager_net(torch):
    """The reference's forward (wavegrad_v190.py) on nn.Conv1d layers: a throw-away float32 module (tools/wavegrad_train_bench.py trains it)."""
    import torch.nn as nn
    import torch.nn.functional as F

    db, fl, ub = YAML["dblock"], YAML["film"], YAML["ublock"]

    def conv(cin, cout, k, d=1, stride=1, same=True):
        return nn.Conv1d(cin, cout, k, stride=stride, dilation=d, padding=(k // 2) * d if same else 0)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.init = conv(1, 32, 5)
            self.d, self.f, self.u = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
            cin = 32
            for hid, fac in zip(db["hidden_size"], db["factor"]):
                self.d.append(nn.ModuleList([conv(cin, hid, 1), conv(hid, hid, fac, stride=fac, same=False),
                                             conv(cin, cin, fac, stride=fac, same=False), conv(cin, hid, 3, 1), conv(hid, hid, 3, 2),
                                             conv(hid, hid, 3, 4)]))
                cin = hid
            cin = 32
            for o in fl["output_size"]:
                self.f.append(nn.ModuleList([conv(cin, cin, 3), conv(cin, 2 * o, 3)]))
                cin = o
            cin = 768
            for hid, dil in zip(ub["hidden_size"], ub["dilation"]):
                self.u.append(nn.ModuleList([conv(cin, hid, 1), conv(cin, hid, 3, dil[0]), conv(hid, hid, 3, dil[1]),
                                             conv(hid, hid, 3, dil[2]), conv(hid, hid, 3, dil[3])]))
                cin = hid
            self.first, self.last = conv(128, 768, 3), conv(128, 1, 3)

        def forward(self, audio, level, spec):
            x = self.init(audio[:, None])
            films = []
            for n, film in enumerate(self.f):
                if n:
                    r, d1, d2, c1, c2, c3 = self.d[n - 1]
                    res = d1(r(x))
                    y = d2(x)
                    for c in (c1, c2, c3):
                        y = c(F.leaky_relu(y, 0.2))
                    x = y + res
                h = F.leaky_relu(film[0](x), 0.2)
                count = h.shape[1] // 2
                e = level[:, None] * torch.exp(-math.log(1e4) * torch.arange(count, device=h.device) / count)[None]
                h = h + torch.cat([e.sin(), e.cos()], -1)[:, :, None]
                films.append(film[1](h).chunk(2, 1))
            x = self.first(spec)
            r2 = 2 ** 0.5
            for blk, fac, (shift, scale) in zip(self.u, ub["factor"], films[::-1]):
                b1 = blk[0](x).repeat_interleave(fac, 2) / fac
                b2 = blk[1](F.leaky_relu(x, 0.2).repeat_interleave(fac, 2) / fac)
                b2 = blk[2](F.leaky_relu((scale * b2 + shift) / r2, 0.2))
                x = (b1 + b2) / r2
                b3 = blk[3](F.leaky_relu((scale * x + shift) / r2, 0.2))
                b3 = blk[4](F.leaky_relu((scale * b3 + shift) / r2, 0.2))
                x = (x + b3) / r2
            return self.last(x)[:, 0]

    return Net()


def eager(a, torch):
    net = eager_net(torch).cuda().eval()
    audio, spec, level = torch.randn((1, 300 * a.frames), device="cuda"), torch.rand((1, 128, a.frames), device="cuda"), torch.tensor([0.5], device="cuda")
    try:
        with torch.no_grad():
            return timed(torch, lambda: net(audio, level, spec), a.warmup, a.repeats)
    except RuntimeError as err:  # e.g. MIOpen refusing a shape: reported as it is
        return {"error": str(err).split("\n")[0][:300]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("ours", "eager_f32"), default="ours")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("wavegrad_bench needs a HIP device: nothing is measured without one")
    torch.manual_seed(0)
    result = {"part": a.part, "frames": a.frames, "steps": a.steps, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    result.update(ours(a, torch) if a.part == "ours" else {"eager_f32_forward": eager(a, torch)})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
