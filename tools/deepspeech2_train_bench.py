#!/usr/bin/env python3
"""DeepSpeech2 training step at the example's training shape: examples/deepspeech2/deepspeech2.yaml (hidden_size 1024,
hidden_layers 5, 161 frequency bins), 64 utterances padded to 1250 frames (T1 = 625 LSTM steps per layer), 100 labels each.

--frontend frozen | trained   models.DeepSpeech2Trainer's option of that name (default frozen), for both parts.
--part ours        models.DeepSpeech2Trainer.step.  One JSON line with
    step / forward / loss / backward / update   median_ms and min_ms of --repeats steps, the phases from device events at the
                   trainer's phase boundaries (forward includes the front end; backward the fc products and every layer)
    loss_value / overflow   what the last step returned;  launches   the trainer's launch counts per phase of one step
    fwd_layer / bwd_layer   one middle layer (K = H) alone: ma_lstm_bidir_train_bf16 (projection GEMMs included) and
                   ma_lstm_bidir_bwd_bf16 (the step launches only) on preallocated buffers
    fwd_step_us / bwd_step_us   those two divided by T1: microseconds per step launch, forward beside backward
    bwd_products   the four products that follow the backward steps of that layer (dW_ih + db, dW_hh, dx), per layer
    tape_mb        ma_lstm_train_tape_bytes per layer;  peak_mem_mb   torch.cuda.max_memory_allocated over the steps
    --frontend trained adds, from device events inside the same steps: frontend_forward (conv1, conv2, both BatchNorms), and the
                   front end's backward split into frontend_batchnorm (both stages' launches), frontend_conv2_dw, frontend_conv2_dx
                   and frontend_conv1_dw; their launch counts are in `launches`
--part eager       the same recurrent stack, fc, CTC loss and Adam step in PyTorch-ROCm eager (torch.nn.LSTM autograd, float32) on the
    output of an untimed front end: median_ms, or {"error": ...} if a library refuses the shape (reported, not worked round).
    With --frontend trained the front end is part of the timed graph: conv2d + batch_norm(training=True) + tanh twice, in float32.
The reference runs on MindSpore, which is not installed here: nothing is said about its speed.  No threshold: the figures are
measurements."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LABELS = 29


def _stat(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3)}


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
    return _stat(ms)


def _batch(a, torch):
    import numpy as np

    g = np.random.RandomState(0)
    x = torch.randn((a.batch, 1, 161, a.frames), device="cuda")
    lengths = np.full(a.batch, a.frames, np.int32)
    targets = g.randint(0, LABELS - 1, (a.batch, a.labels)).astype(np.int32)
    return x, lengths, targets, np.full(a.batch, a.labels, np.int32)


def ours(a, torch):
    from mindaudio_amd import _host, _lib, ops
    from mindaudio_amd.models import DeepSpeech2Trainer, DeepSpeechModel

    _host.require_gpu()
    lib = _lib.load()
    model = DeepSpeechModel(a.batch, ["x"] * LABELS, a.hidden, a.layers, dict(sample_rate=16000, window_size=0.02)).cuda().eval()
    trainer = DeepSpeech2Trainer(model, 3e-4, 1e-5, loss_scale=1024, frontend=a.frontend)
    x, lengths, targets, target_lengths = _batch(a, torch)
    torch.cuda.reset_peak_memory_stats()
    for _ in range(a.warmup):
        trainer.step(x, lengths, targets, target_lengths)
    phases = {k: [] for k in ("step", "forward", "loss", "backward", "update")}
    # (name of a piece of the trained front end: the event pairs whose spans add up to it)
    pieces = {"frontend_forward": [("start", "fe_stage2")], "frontend_batchnorm": [("lstm_backward", "fe_bn2_bwd"), ("fe_conv2_dx", "fe_bn1_bwd")],
              "frontend_conv2_dw": [("fe_bn2_bwd", "fe_conv2_dw")], "frontend_conv2_dx": [("fe_conv2_dw", "fe_conv2_dx")],
              "frontend_conv1_dw": [("fe_bn1_bwd", "fe_conv1_dw")]} if a.frontend == "trained" else {}
    phases.update({k: [] for k in pieces})
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        trainer.events = []
        loss, overflow = trainer.step(x, lengths, targets, target_lengths)
        torch.cuda.synchronize()
        ev = dict(trainer.events)
        order = ["start", "forward", "loss", "backward", "update"]
        for prev, name in zip(order, order[1:]):
            phases[name].append(ev[prev].elapsed_time(ev[name]))
        phases["step"].append(ev["start"].elapsed_time(ev["update"]))
        for name, spans in pieces.items():
            phases[name].append(sum(ev[lo].elapsed_time(ev[hi]) for lo, hi in spans))
    trainer.events = None
    out = {k: _stat(v) for k, v in phases.items()}
    out.update(loss_value=round(float(loss), 4), overflow=bool(overflow), launches=dict(trainer.launches),
               peak_mem_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
    # one middle layer alone
    T1, B, H = (a.frames - 1) // 2 + 1, a.batch, a.hidden
    L = model._prepared["layers"][-1]
    out["tape_mb"] = round(lib.ma_lstm_train_tape_bytes(T1, B, H) / 2 ** 20, 1)
    hb = torch.randn((T1, B, H), device="cuda").mul_(0.1).to(torch.bfloat16)
    nbytes = int(lib.ma_lstm_workspace_bytes(T1, B, H, T1))
    bufs = dict(workspace=torch.empty((nbytes,), dtype=torch.uint8, device="cuda"), out_f32=torch.empty((T1, B, H), device="cuda"),
                out_bf16=torch.empty((T1, B, H), dtype=torch.bfloat16, device="cuda"),
                tape_buf=torch.empty((int(lib.ma_lstm_train_tape_bytes(T1, B, H)),), dtype=torch.uint8, device="cuda"))
    reps = max(3, a.repeats // 2)
    out["fwd_layer"] = timed(torch, lambda: ops.lstm_bidir_train(hb, L, chunk=T1, **bufs), 1, reps)
    _, _, tape = ops.lstm_bidir_train(hb, L, chunk=T1, **bufs)
    dout = torch.randn((T1, B, H), device="cuda")
    dg = torch.empty((2, T1, B, 4 * H), dtype=torch.bfloat16, device="cuda")
    wsb = int(lib.ma_lstm_bwd_workspace_bytes(B, H))
    ws = torch.empty((wsb,), dtype=torch.uint8, device="cuda")
    out["bwd_layer"] = timed(torch, lambda: _lib.check(lib.ma_lstm_bidir_bwd_bf16(
        dout.data_ptr(), T1, B, H, tape.buf.data_ptr(), tape.buf.numel(), L["whh_bwd"].data_ptr(), 3, dg.data_ptr(), ws.data_ptr(), wsb, None),
        "lstm_bwd"), 1, reps)
    whole = timed(torch, lambda: ops.lstm_bidir_backward(dout, tape, L, dgates=dg), 1, reps)
    out["bwd_products"] = {k: round(whole[k] - out["bwd_layer"][k], 3) for k in whole}
    out["fwd_step_us"] = round(out["fwd_layer"]["median_ms"] * 1e3 / T1, 3)
    out["bwd_step_us"] = round(out["bwd_layer"]["median_ms"] * 1e3 / T1, 3)
    return out


def eager(a, torch):
    import torch.nn.functional as F

    from mindaudio_amd.models import DeepSpeechModel

    model = DeepSpeechModel(a.batch, ["x"] * LABELS, a.hidden, a.layers, dict(sample_rate=16000, window_size=0.02)).cuda().eval()
    x, lengths, targets, target_lengths = _batch(a, torch)
    xin = model.frontend(x)[:, :, :model.rnn_input_size].float()  # the frozen front end, untimed
    T1 = xin.shape[0]
    trained = a.frontend == "trained"
    convs = [torch.nn.Conv2d(1, 32, (41, 11), stride=(2, 2), padding=(20, 5), bias=False).cuda(),
             torch.nn.Conv2d(32, 32, (21, 11), stride=(2, 1), padding=(10, 5), bias=False).cuda()] if trained else []
    norms = [torch.nn.BatchNorm2d(32, momentum=0.1).cuda().train() for _ in convs]
    lstms = [torch.nn.LSTM(model.rnn_input_size if k == 0 else a.hidden, a.hidden, bidirectional=True).cuda() for k in range(a.layers)]
    fc = torch.nn.Linear(a.hidden, LABELS, bias=False).cuda()
    params = [p for m in lstms + [fc] + convs + norms for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5)
    ys, ylens = torch.from_numpy(targets).long().cuda(), torch.from_numpy(target_lengths).long().cuda()
    hlens = torch.full((a.batch,), T1, dtype=torch.long, device="cuda")

    def step():
        h = xin
        if trained:  # (B, 1, F, T) -> (B, 32, F2, T1) -> (T1, B, 32 F2)
            h = x
            for conv, norm in zip(convs, norms):
                h = torch.tanh(norm(conv(h)))
            h = h.reshape(a.batch, -1, T1).permute(2, 0, 1)
        for lstm in lstms:
            h, _ = lstm(h)
            h = h.reshape(T1, a.batch, 2, -1).sum(2)
        loss = F.ctc_loss(torch.log_softmax(fc(h), -1), ys, hlens, ylens, blank=LABELS - 1, reduction="sum", zero_infinity=True) / a.batch
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    try:
        torch.cuda.reset_peak_memory_stats()
        out = timed(torch, step, a.warmup, a.repeats)
        out["peak_mem_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        return out
    except RuntimeError as err:  # e.g. MIOpen refusing the shape: reported as it is
        return {"error": str(err).split("\n")[0][:300]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("ours", "eager"), default="ours")
    ap.add_argument("--frontend", choices=("frozen", "trained"), default="frozen")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--labels", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("deepspeech2_train_bench needs a HIP device: nothing is measured without one")
    torch.manual_seed(0)
    result = {"part": a.part, "frontend": a.frontend, "batch": a.batch, "frames": a.frames, "hidden": a.hidden, "layers": a.layers, "labels": a.labels,
              "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    result.update(ours(a, torch) if a.part == "ours" else {"eager": eager(a, torch)})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
