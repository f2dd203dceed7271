#!/usr/bin/env python3
"""FastSpeech2 at the example's shape: examples/fastspeech2/fastspeech2.yaml on --batch sentences of --phonemes phonemes, random weights
with the duration head's bias at log 8 (about 7 frames a phoneme, so 100 phonemes give about 700 mel frames).

--part ours        prints one JSON line; medians (with min / max) of --repeats runs after --warmup runs
    infer          the whole FastSpeech2.infer, wall clock (it holds the one read-back, mel_len)
    encoder, expanded_encoder, decoder   each ma_fs2_fft_stack call, device events inside an infer
    adaptor        infer minus the three stacks (embeddings, predictors, heads, length regulator, mel_linear, the read-back)
    attention      one ma_mha_d128_bf16 launch at the decoder's shape (B, frames, 2 heads of 128), device events
    launches_per_infer, frames, peak_mem_mb (torch.cuda.max_memory_allocated over an infer)
--part eager_f32   the same network written with PyTorch-ROCm eager ops in float32 (embedding, scaled_dot_product_attention under the
                   key-padding mask, group_norm, conv1d, layer_norm, searchsorted, repeat_interleave) on the same GPU and the same
                   weights: one infer, wall clock, or {"error": ...} if a library refuses a shape.
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

YAML = dict(use_fp16=False, n_mels=128, hop_samples=300, n_fft=2048, sample_rate=22050,
            pitch=dict(feature="frame_level", pitch_min=0.0, pitch_max=843.436831),
            energy=dict(feature="frame_level", energy_min=0.0436493270, energy_max=494.149902),
            model=dict(n_src_vocab=360, max_seq_len=1000,
                       transformer=dict(encoder_layer=4, encoder_head=2, encoder_hidden=256, decoder_layer=4, decoder_head=2,
                                        decoder_hidden=256, conv_filter_size=1024, conv_kernel_size=[9, 1]),
                       variance_predictor=dict(filter_size=256, kernel_size=3),
                       variance_embedding=dict(pitch_quantization="log", energy_quantization="linear", n_bins=256)))


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _wall_ms(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _model(torch):
    from mindaudio_amd.models import FastSpeech2

    torch.manual_seed(0)
    model = FastSpeech2(YAML)
    with torch.no_grad():
        model.variance_adaptor.duration_predictor.linear_layer.bias.fill_(math.log(8.0))
    return model.cuda().eval()


def _inputs(torch, a):
    g = torch.Generator().manual_seed(1)
    texts = torch.randint(1, 361, (a.batch, a.phonemes), generator=g)
    return texts, torch.full((a.batch,), a.phonemes, dtype=torch.int64)


def ours(a, torch):
    from mindaudio_amd import _host, _lib

    _host.require_gpu()
    lib = _lib.load()
    model = _model(torch)
    texts, lens = _inputs(torch, a)
    spans = {}
    inner = model._stack

    def timed_stack(lib_, name, *rest):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        inner(lib_, name, *rest)
        e.record()
        spans.setdefault(name, []).append((s, e))

    model._stack = timed_stack
    run = lambda: model.infer(None, texts, lens, a.phonemes)
    for _ in range(a.warmup):
        out = run()
    spans.clear()
    torch.cuda.reset_peak_memory_stats()
    walls = [_wall_ms(torch, run) for _ in range(a.repeats)]
    res = {"infer": _stats(walls), "frames": int(out["mel_predictions"].shape[1]), "launches_per_infer": model.launches,
           "peak_mem_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    stacks = 0.0
    for name, evs in spans.items():
        res[name] = _stats([s.elapsed_time(e) for s, e in evs])
        stacks += res[name]["median_ms"]
    res["adaptor"] = {"median_ms": round(res["infer"]["median_ms"] - stacks, 4)}
    # the attention launch alone at the decoder's shape
    B, T, C = a.batch, res["frames"], 256
    qkv = torch.randn((B * T, 3 * C), device="cuda").to(torch.bfloat16)
    ctx = torch.empty((B * T, C), dtype=torch.bfloat16, device="cuda")
    ln = torch.full((B,), T, dtype=torch.int32, device="cuda")
    base = qkv.data_ptr()

    def attn():
        _lib.check(lib.ma_mha_d128_bf16(base, 3 * C, base + 2 * C, 3 * C, base + 4 * C, 3 * C, ln.data_ptr(), B, T, T, 2, 128,
                                        1.0 / math.sqrt(128.0), ctx.data_ptr(), C, T, None), "mha")

    ms = []
    for i in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        attn()
        e.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(s.elapsed_time(e))
    res["attention"] = _stats(ms)
    res["attention_tflops"] = round(4.0 * B * 2 * T * T * 128 / (res["attention"]["median_ms"] * 1e-3) / 1e12, 3)
    return res


def eager(a, torch):
    """FastSpeech2.infer with eager float32 ops on the model's own weights."""
    import torch.nn.functional as F

    model = _model(torch)
    sd = {k: v.float() for k, v in model.state_dict().items()}
    pos = model.position_enc.float()
    texts, lens = _inputs(torch, a)
    texts, lens = texts.cuda(), lens.cuda()

    def block(x, p, key_mask, heads):
        B, T, C = x.shape
        w = lambda n: sd[p + n]
        q, k, v = (F.linear(x, w("slf_attn.%s.weight" % n), w("slf_attn.%s.bias" % n)).view(B, T, heads, C // heads).transpose(1, 2)
                   for n in ("w_qs", "w_ks", "w_vs"))
        ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=~key_mask[:, None, None, :]).transpose(1, 2).reshape(B, T, C)
        y = F.linear(ctx, w("slf_attn.fc.weight"), w("slf_attn.fc.bias")) + x
        keep = (~key_mask).float()[:, :, None]
        x = F.group_norm(y.transpose(1, 2), 8, w("slf_attn.layer_norm.gamma"), w("slf_attn.layer_norm.beta")).transpose(1, 2) * keep
        hcur = F.relu(F.conv1d(x.transpose(1, 2), w("pos_ffn.w_1.weight"), w("pos_ffn.w_1.bias"), padding=4))
        y = F.conv1d(hcur, w("pos_ffn.w_2.weight"), w("pos_ffn.w_2.bias")).transpose(1, 2) + x
        return F.group_norm(y.transpose(1, 2), 8, w("pos_ffn.layer_norm.gamma"), w("pos_ffn.layer_norm.beta")).transpose(1, 2) * keep

    def stack(name, x, key_mask, layers=4):
        for n in range(layers):
            x = block(x, "%s.layer_stack.%d." % (name, n), key_mask, 2)
        return x

    def predictor(name, x):
        p = "variance_adaptor.%s." % name
        w = lambda n: sd[p + n]
        hcur = F.relu(F.conv1d(x.transpose(1, 2), w("conv1.0.weight"), w("conv1.0.bias"), padding=1)).transpose(1, 2)
        hcur = F.layer_norm(hcur, (256,), w("norm1.gamma"), w("norm1.beta"), 1e-7)
        hcur = F.relu(F.conv1d(hcur.transpose(1, 2), w("conv2.0.weight"), w("conv2.0.bias"), padding=1)).transpose(1, 2)
        hcur = F.layer_norm(hcur, (256,), w("norm2.gamma"), w("norm2.beta"), 1e-7)
        return F.linear(hcur, w("linear_layer.weight"), w("linear_layer.bias"))[..., 0]

    def infer():
        B, Ts = texts.shape
        x = F.embedding(texts, sd["encoder.src_word_emb.weight"]) + pos[None, :Ts]
        x = stack("encoder", x, texts == 0)
        logd = predictor("duration_predictor", x) * (texts != 0).float()
        dur = torch.clamp(torch.round(torch.exp(logd) - 1), min=0).long()
        rows = [torch.repeat_interleave(texts[b], dur[b]) for b in range(B)]
        ids = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True)
        T = ids.shape[1]
        x = F.embedding(ids, sd["expanded_encoder.src_word_emb.weight"]) + pos[None, :T]
        x = stack("expanded_encoder", x, ids == 0)
        pitch = predictor("pitch_predictor", x)
        x = x + F.embedding(torch.searchsorted(sd["variance_adaptor.pitch_bins"], pitch), sd["variance_adaptor.pitch_embedding.weight"])
        energy = predictor("energy_predictor", x)
        x = x + F.embedding(torch.searchsorted(sd["variance_adaptor.energy_bins"], energy), sd["variance_adaptor.energy_embedding.weight"])
        x = stack("decoder", x + pos[None, :T], ids == 0)
        return F.linear(x, sd["mel_linear.weight"], sd["mel_linear.bias"])

    try:
        with torch.no_grad():
            for _ in range(a.warmup):
                mel = infer()
            return dict(_stats([_wall_ms(torch, infer) for _ in range(a.repeats)]), frames=int(mel.shape[1]))
    except RuntimeError as err:  # e.g. MIOpen refusing a shape: reported as it is
        return {"error": str(err).split("\n")[0][:300]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("ours", "eager_f32"), default="ours")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--phonemes", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("fastspeech2_bench needs a HIP device: nothing is measured without one")
    result = {"part": a.part, "batch": a.batch, "phonemes": a.phonemes, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    result.update(ours(a, torch) if a.part == "ours" else {"eager_f32_infer": eager(a, torch)})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
