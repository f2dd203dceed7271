#!/usr/bin/env python3
"""TasNet forward at the example's evaluation shape: examples/tasnet/tasnet.yaml (L 40, N 500, hidden_size 512, num_layers 4, nspk 2) on
--batch utterances of 3320 segments, under both LSTM schedules.

--part ours        prints one JSON line; every timing is {median_ms, min_ms, max_ms} of --repeats device-event timings after --warmup
                   runs, the two schedules ALTERNATING inside each repeat so that drift hits both alike
    forward        {pipelined, layered}: TasNet.forward, every launch included
    lstm           {pipelined, layered}: the LSTM stack alone on the buffers of a forward
    diagonal_us    pipelined lstm / (K + layers - 1): the mean time of one diagonal launch (up to layers * H / 16 workgroups)
    step_us        layered lstm / (layers * K): the mean time of one layered step, the projection GEMMs included
    encoder / fc / decode   the gated-encoder launch, the fc GEMM and the mask + decode launch, each alone
    launch_gap_us  the mean time per launch of 2000 back-to-back launches of a near-empty kernel (ma_valu_issue_probe, one iteration,
                   one 4-wave workgroup per CU; a diagonal has at most layers * H / 16 workgroups, a layered step H / 16): what a launch
                   costs when the kernel does nothing
    agreement      relative rms between the two schedules' outputs on the timed input
    peak_mem_mb    torch.cuda.max_memory_allocated over a forward (weights, workspaces and the input included)
--part eager_f32   torch.nn.LSTM(N, hidden, num_layers) in PyTorch-ROCm eager, float32, on the same GPU and the same (K, batch, N) input:
                   {median_ms, ...}, or {"error": ...} if the library refuses the shape (reported, not worked round).
Each part is a process of its own so that a job script can give each its own time limit.
The reference itself runs on MindSpore, which is not installed here: nothing is said about its speed.  No threshold: the figures
are measurements."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _once(torch, fn):
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def timed(torch, fns, warmup, repeats):
    """{name: stats}: the functions of `fns` take turns inside every repeat."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(_once(torch, fn))
    return {k: _stats(v) for k, v in ms.items()}


def ours(a, torch):
    from mindaudio_amd import _host, _lib
    from mindaudio_amd.models import TasNet

    _host.require_gpu()
    lib = _lib.load()
    model = TasNet(a.L, a.N, a.hidden, a.layers, nspk=a.nspk).cuda().eval()
    x = 0.1 * torch.randn((a.batch, a.segments, a.L), device="cuda")
    K = a.segments

    def forward(schedule):
        model.schedule = schedule
        return model(x)

    torch.cuda.reset_peak_memory_stats()
    ref = {s: forward(s).clone() for s in ("pipelined", "layered")}
    torch.cuda.synchronize()
    out = {"peak_mem_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    d = (ref["pipelined"] - ref["layered"]).double()
    out["agreement"] = float((d.pow(2).mean().sqrt() / ref["layered"].double().pow(2).mean().sqrt()).cpu())
    out["forward"] = timed(torch, {s: (lambda s=s: forward(s)) for s in ("pipelined", "layered")}, a.warmup, a.repeats)
    mw, coef, xin = model.encode(x)
    out["lstm"] = timed(torch, {s: (lambda s=s: model.lstm_stack(xin, s)) for s in ("pipelined", "layered")}, a.warmup, a.repeats)
    out["diagonal_us"] = round(out["lstm"]["pipelined"]["median_ms"] * 1e3 / (K + a.layers - 1), 3)
    out["step_us"] = round(out["lstm"]["layered"]["median_ms"] * 1e3 / (a.layers * K), 3)
    _, hb = model.lstm_stack(xin)
    parts = timed(torch, {"encoder": lambda: model.encode(x), "fc_and_decode": lambda: model.decode(hb, mw, coef)}, a.warmup, a.repeats)
    out["encoder"] = parts["encoder"]
    P, ws = model._prepared, next(w for w in model._ws.values() if w["mw"] is mw)
    est = torch.empty((a.batch, a.nspk, K, a.L), device="cuda")
    out["decode"] = timed(torch, {"decode": lambda: _lib.check(lib.ma_tasnet_mask_decode_f32(
        ws["score"].data_ptr(), ws["ld"], mw.data_ptr(), coef.data_ptr(), a.batch, K, a.nspk, a.N, P["basis"].data_ptr(),
        P["basis_bias"].data_ptr(), a.L, est.data_ptr(), None), "decode")}, a.warmup, a.repeats)["decode"]
    out["fc"] = {k: round(parts["fc_and_decode"][k] - out["decode"][k], 4) for k in ("median_ms",)}
    sink = torch.zeros((1 << 16,), device="cuda")
    n = 2000

    def launches():
        for _ in range(n):
            lib.ma_valu_issue_probe(1, 1, sink.data_ptr(), None)

    gap = timed(torch, {"gap": launches}, 1, max(5, a.repeats))["gap"]
    out["launch_gap_us"] = {k.replace("_ms", ""): round(v * 1e3 / n, 3) for k, v in gap.items()}
    out["workgroups"] = {"diagonal": a.layers * a.hidden // 16, "layered_step": a.hidden // 16}
    return out


def eager(a, torch):
    lstm = torch.nn.LSTM(a.N, a.hidden, a.layers).cuda().eval()
    x = torch.randn((a.segments, a.batch, a.N), device="cuda")
    try:
        with torch.no_grad():
            return timed(torch, {"lstm": lambda: lstm(x)}, a.warmup, a.repeats)["lstm"]
    except RuntimeError as err:  # e.g. MIOpen refusing the shape: reported as it is
        return {"error": str(err).split("\n")[0][:300]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("ours", "eager_f32"), default="ours")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--segments", type=int, default=3320)
    ap.add_argument("--L", type=int, default=40)
    ap.add_argument("--N", type=int, default=500)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--nspk", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tasnet_bench needs a HIP device: nothing is measured without one")
    torch.manual_seed(0)
    result = {"part": a.part, "batch": a.batch, "segments": a.segments, "L": a.L, "N": a.N, "hidden": a.hidden, "layers": a.layers,
              "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    result.update(ours(a, torch) if a.part == "ours" else {"eager_f32_lstm": eager(a, torch)})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
