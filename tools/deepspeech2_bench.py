#!/usr/bin/env python3
"""DeepSpeech2 forward at the example's evaluation shape: examples/deepspeech2/deepspeech2.yaml (hidden_size 1024, hidden_layers 5,
sample rate 16000 -> 161 frequency bins) on 128 utterances padded to 3500 frames (T1 = 1750 LSTM steps per layer).

--part ours        prints one JSON line with
    forward        median_ms / min_ms of --repeats device-event timings of DeepSpeechModel.forward (every launch included)
    front_end / lstm / fc   the same for the three parts, each timed alone on the buffers of a forward
    conv1          the first convolution's launch alone (the rest of front_end is conv2's calls, one per output frequency)
    step_us        lstm time / (layers * T1): the mean time of one recurrent step, projection GEMMs included
    step_only_us   one layer's step launches alone (time_chunk = T1, the projection GEMM timed separately and subtracted)
    launch_gap_us  the mean time per launch of 2000 back-to-back launches of a near-empty kernel with a step's grid size
                   (ma_valu_issue_probe, one iteration): what a launch per step costs when the kernel does nothing
    peak_mem_mb    torch.cuda.max_memory_allocated over a forward (weights, workspaces and the input included)
--part eager_f32 / eager_bf16   the same network in PyTorch-ROCm eager (torch.nn.LSTM, torch.nn.functional.conv2d) on the same GPU,
    float32 or under bf16 autocast: median_ms, or {"error": ...} if the library refuses the shape (reported, not worked round).
Each part is a process of its own so that a job script can give each its own time limit.
The reference itself runs on MindSpore, which is not installed here: nothing is said about its speed.  No threshold: the figures
are measurements."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LABELS = 29


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(end))
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3)}


def ours(a, torch):
    import ctypes

    from mindaudio_amd import _host, _lib
    from mindaudio_amd.models import DeepSpeechModel

    _host.require_gpu()
    lib = _lib.load()
    model = DeepSpeechModel(a.batch, ["x"] * LABELS, a.hidden, a.layers, dict(sample_rate=16000, window_size=0.02)).cuda().eval()
    x = torch.randn((a.batch, 1, 161, a.frames), device="cuda")
    lengths = [a.frames] * a.batch
    torch.cuda.reset_peak_memory_stats()
    model(x, lengths)
    torch.cuda.synchronize()
    out = {"peak_mem_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    out["forward"] = timed(torch, lambda: model(x, lengths), a.warmup, a.repeats)
    out["front_end"] = timed(torch, lambda: model.frontend(x), a.warmup, a.repeats)
    xin = model.frontend(x)
    P, fws = model._prepared, next(w for w in model._ws.values() if w["xin"] is xin)
    out["conv1"] = timed(torch, lambda: _lib.check(lib.ma_ds2_conv1_bf16(
        x.data_ptr(), a.batch, 161, a.frames, P["w1t"].data_ptr(), P["scale1"].data_ptr(), P["shift1"].data_ptr(), fws["Fpad"],
        fws["act1"].data_ptr(), None), "conv1"), a.warmup, a.repeats)  # (conv2 = front_end - conv1: 41 calls)
    out["lstm"] = timed(torch, lambda: model.lstm_stack(xin), a.warmup, a.repeats)
    T1, B, H = xin.shape[0], a.batch, a.hidden
    out["step_us"] = round(out["lstm"]["median_ms"] * 1e3 / (a.layers * T1), 3)
    _, hb = model.lstm_stack(xin)
    fcw = model._prepared["fc"]
    logits = torch.empty((T1 * B, 32), device="cuda")
    e = _lib.GemmEpilogue()
    e.alpha = 1.0
    out["fc"] = timed(torch, lambda: _lib.check(lib.ma_gemm_bf16(hb.data_ptr(), H, fcw.data_ptr(), H, logits.data_ptr(), 32, T1 * B, LABELS,
                                                                 H, ctypes.byref(e), None), "fc"), a.warmup, a.repeats)
    # one layer (the second: K = H) with the whole projection in one chunk, and that projection alone
    L = model._prepared["layers"][-1]
    nbytes = lib.ma_lstm_workspace_bytes(T1, B, H, T1)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    of, ob = torch.empty((T1, B, H), device="cuda"), torch.empty((T1, B, H), dtype=torch.bfloat16, device="cuda")
    layer = timed(torch, lambda: _lib.check(lib.ma_lstm_bidir_bf16(hb.data_ptr(), T1, B, H, H, L["wih"].data_ptr(), L["whh"].data_ptr(),
                                                                   L["bias"].data_ptr(), 3, T1, of.data_ptr(), ob.data_ptr(), None,
                                                                   ws.data_ptr(), nbytes, None), "lstm"), 1, max(3, a.repeats // 2))
    proj = torch.empty((T1 * B, 4 * H), device="cuda")
    e.bias = L["bias"].data_ptr()
    gemm = timed(torch, lambda: _lib.check(lib.ma_gemm_bf16(hb.data_ptr(), H, L["wih"].data_ptr(), H, proj.data_ptr(), 4 * H, T1 * B, 4 * H,
                                                            H, ctypes.byref(e), None), "proj"), 1, max(3, a.repeats // 2))
    out["one_layer"], out["one_projection_gemm"] = layer, gemm
    out["step_only_us"] = round((layer["median_ms"] - 2 * gemm["median_ms"]) * 1e3 / T1, 3)
    sink = torch.zeros((1 << 16,), device="cuda")
    n = 2000

    def launches():
        for _ in range(n):
            lib.ma_valu_issue_probe(1, 1, sink.data_ptr(), None)

    gap = timed(torch, launches, 1, 5)
    out["launch_gap_us"] = round(gap["median_ms"] * 1e3 / n, 3)
    out["recurrent_gflop_per_step"] = round(2 * 2 * B * 4 * H * H / 1e9, 3)
    return out


def eager(a, torch, bf16):
    import torch.nn.functional as F

    dev = "cuda"
    conv1 = torch.nn.Conv2d(1, 32, (41, 11), stride=(2, 2), padding=(20, 5), bias=False).to(dev)
    conv2 = torch.nn.Conv2d(32, 32, (21, 11), stride=(2, 1), padding=(10, 5), bias=False).to(dev)
    bn1, bn2 = torch.nn.BatchNorm2d(32).to(dev).eval(), torch.nn.BatchNorm2d(32).to(dev).eval()
    lstms = [torch.nn.LSTM(1312 if k == 0 else a.hidden, a.hidden, bidirectional=True).to(dev) for k in range(a.layers)]
    fc = torch.nn.Linear(a.hidden, LABELS, bias=False).to(dev)
    x = torch.randn((a.batch, 1, 161, a.frames), device=dev)

    def forward():
        y = torch.tanh(bn2(conv2(torch.tanh(bn1(conv1(x))))))
        b, c, f, t = y.shape
        h = y.reshape(b, c * f, t).permute(2, 0, 1)
        for lstm in lstms:
            h, _ = lstm(h)
            h = h.reshape(t, b, 2, -1).sum(2)
        return fc(h)

    try:
        with torch.no_grad():
            if bf16:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return timed(torch, forward, a.warmup, a.repeats)
            return timed(torch, forward, a.warmup, a.repeats)
    except RuntimeError as err:  # e.g. MIOpen refusing the shape: reported as it is
        return {"error": str(err).split("\n")[0][:300]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("ours", "eager_f32", "eager_bf16"), default="ours")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--frames", type=int, default=3500)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("deepspeech2_bench needs a HIP device: nothing is measured without one")
    torch.manual_seed(0)
    result = {"part": a.part, "batch": a.batch, "frames": a.frames, "hidden": a.hidden, "layers": a.layers, "repeats": a.repeats,
              "device": torch.cuda.get_device_name(0)}
    result.update(ours(a, torch) if a.part == "ours" else {a.part: eager(a, torch, a.part == "eager_bf16")})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
