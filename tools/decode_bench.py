#!/usr/bin/env python3
"""Decode modes at bench.py's headline workload: 64 x 10 s synthetic waveforms -> fbank -> hybrid Conformer (the shipped shapes:
d 256, 12 encoder blocks, 6 decoder blocks, V = 4233) -> CTC greedy search / CTC prefix beam search (beam 10) / attention rescoring
(beam 10).  Prints per-stage device time (CUDA events, median of --reps), utterances/s of each mode end to end, and the host-side
baseline: the reference's prefix search restated in Python (utils/recognize.py:273-336) on the same top-k lists.

The weights are random, so the CTC head's blank bias is calibrated first: 10 % of the frames are non-blank, about 25 tokens per 10 s
utterance (a trained Chinese model's rate); without it the hypotheses of a random head run to hundreds of tokens.

--arm attention measures the autoregressive `attention` decode mode instead, for ONE 10 s utterance at the same model and beam 10:
the device-resident search (KV-cached decoder step + beam step, conformer.asr_model.recognize), its kernel launches per step, the same
search done by re-running TransformerDecoder on the growing prefix at every step (what the reference does, minus its maxlen padding
and its repeated encoder output; this yardstick lives here only) and attention_rescoring on the same input.  With random weights no
beam ever takes eos, so both searches run to the length limit (248 steps): the per-step figures are the ones to carry over.

usage: python tools/decode_bench.py [--reps 10] [--host-utts 4] [--arm ctc|attention]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, SAMPLES, FRAMES, VOCAB, BEAM = 64, 160000, 1000, 4233, 10


def host_prefix_search(lp, ix, beam):
    """utils/recognize.py:273-336 over one utterance's top-k lists (lists of floats / ints per frame)."""
    def log_add(args):
        if all(a == -math.inf for a in args):
            return -math.inf
        m = max(args)
        return m + math.log(sum(math.exp(a - m) for a in args))

    cur = [((), (0.0, -math.inf))]
    for lps, ids in zip(lp, ix):
        nxt = {}
        for ps, s in zip(lps, ids):
            for prefix, (pb, pnb) in cur:
                last = prefix[-1] if prefix else None
                if s == 0:
                    a, b = nxt.get(prefix, (-math.inf, -math.inf))
                    nxt[prefix] = (log_add([a, pb + ps, pnb + ps]), b)
                elif s == last:
                    a, b = nxt.get(prefix, (-math.inf, -math.inf))
                    nxt[prefix] = (a, log_add([b, pnb + ps]))
                    a, b = nxt.get(prefix + (s,), (-math.inf, -math.inf))
                    nxt[prefix + (s,)] = (a, log_add([b, pb + ps]))
                else:
                    a, b = nxt.get(prefix + (s,), (-math.inf, -math.inf))
                    nxt[prefix + (s,)] = (a, log_add([b, pb + ps, pnb + ps]))
        cur = sorted(nxt.items(), key=lambda kv: log_add(list(kv[1])), reverse=True)[:beam]
    return [(p, log_add(list(v))) for p, v in cur]


def attention_arm(a):
    import torch

    import mindaudio_amd as ma
    from mindaudio_amd.conformer.asr_model import (Attention, AttentionRescoring, CTCPrefixBeamSearch, attention_rescoring,
                                                   create_asr_model, recognize)

    dev = torch.device("cuda")
    torch.manual_seed(777)
    model = create_asr_model(80, VOCAB, dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12), ctc_weight=0.3,
                             decoder_conf=dict(attention_heads=4, linear_units=2048, num_blocks=6)).to(dev).eval()
    x = torch.from_numpy((0.1 * np.random.RandomState(1234).randn(1, SAMPLES)).astype(np.float32)).to(dev)
    xs = ma.fbank(x, n_mels=80, n_fft=512, hop_length=160).transpose(1, 2)[:, :FRAMES].contiguous()
    masks = torch.ones(1, 1, FRAMES, device=dev)
    eos = VOCAB - 1
    net = Attention(model, BEAM, eos)
    init = (np.array([eos], np.int32), np.zeros((1, 1), np.int32), np.array([0.0] + [-np.inf] * (BEAM - 1), np.float32),
            np.zeros(BEAM, np.float32))

    class FullPrefix:
        """The yardstick: every step re-runs the decoder on the whole prefix of every beam (beam reorder by gathering token rows)."""
        beam_size = BEAM

        def begin(self, xs_pad, xs_masks, xs_lengths=None):
            sub = xs_masks[:, :, :-2:2][:, :, :-2:2].contiguous()
            enc, enc_mask = model.encoder(xs_pad, sub, sub)
            maxlen = enc.shape[1]
            toks = torch.zeros((BEAM, maxlen), dtype=torch.int32, device=dev)
            tril = torch.tril(torch.ones(maxlen, maxlen, device=dev))

            def step(tokens, t, parent=None):
                if parent is not None:
                    toks[:, :t] = toks[parent.long(), :t]
                toks[:, t] = tokens
                m = tril[:t + 1, :t + 1][None].expand(BEAM, t + 1, t + 1).contiguous()
                return model.decoder.score_hypotheses(enc, enc_mask, toks[:, :t + 1].contiguous(), m, BEAM)[:, t]

            return maxlen, step

    def wall(fn, reps):
        ts, out = [], None
        for r in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if r >= 1:
                ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), out

    sub = masks[:, :, :-2:2][:, :, :-2:2].contiguous()
    enc_ms, (enc, _) = wall(lambda: model.encoder(xs, sub, sub), a.reps)
    steps = enc.shape[1] - 1
    cached_ms, (hyp_c, score_c) = wall(lambda: recognize(net, xs, masks, *init, BEAM, eos), a.reps)
    full_ms, (hyp_f, score_f) = wall(lambda: recognize(FullPrefix(), xs, masks, *init, BEAM, eos), max(1, a.reps // 3))
    ctc, rescore = CTCPrefixBeamSearch(model, BEAM), AttentionRescoring(model, BEAM)
    resc_ms, _ = wall(lambda: attention_rescoring(ctc, rescore, xs, masks, None, eos, eos, BEAM, 0.0), a.reps)
    same = int((hyp_c[0] == hyp_f[0]).sum())
    print(json.dumps({
        "workload": "1 x 10 s synthetic, hybrid Conformer (12 + 6 blocks, V %d), attention decode mode, beam %d" % (VOCAB, BEAM),
        "decoder_steps": steps, "launches_per_step": model.decoder.launches_per_step + 2,
        "encoder_ms": round(enc_ms, 3),
        "attention_ms_per_utt": round(cached_ms, 3), "attention_ms_per_step": round((cached_ms - enc_ms) / steps, 4),
        "full_prefix_ms_per_utt": round(full_ms, 3), "full_prefix_ms_per_step": round((full_ms - enc_ms) / steps, 4),
        "speedup_over_full_prefix": round(full_ms / cached_ms, 2),
        "attention_rescoring_ms_per_utt": round(resc_ms, 3),
        "tokens_equal_to_full_prefix": "%d/%d" % (same, steps), "best_score": [round(float(score_c[0]), 3), round(float(score_f[0]), 3)],
    }))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-utts", type=int, default=4)
    ap.add_argument("--arm", choices=("ctc", "attention"), default="ctc")
    a = ap.parse_args()
    if a.arm == "attention":
        return attention_arm(a)

    import torch

    import mindaudio_amd as ma
    from mindaudio_amd import ops
    from mindaudio_amd.conformer.asr_model import AttentionRescoring, CTCPrefixBeamSearch, create_asr_model, decoder_input

    dev = torch.device("cuda")
    torch.manual_seed(777)
    model = create_asr_model(80, VOCAB, dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=12), ctc_weight=0.3,
                             decoder_conf=dict(attention_heads=4, linear_units=2048, num_blocks=6)).to(dev).eval()
    x = torch.from_numpy((0.1 * np.random.RandomState(1234).randn(BATCH, SAMPLES)).astype(np.float32)).to(dev)
    masks = torch.ones(BATCH, 1, FRAMES, device=dev)
    sub = masks[:, :, :-2:2][:, :, :-2:2].contiguous()
    eos = VOCAB - 1

    def encode():
        feats = ma.fbank(x, n_mels=80, n_fft=512, hop_length=160)
        xs = feats.transpose(1, 2)[:, :FRAMES]
        return model.encoder(xs, sub, sub)

    enc, enc_mask = encode()
    b, t2, _ = enc.shape
    with torch.no_grad():  # blank bias: the 90th percentile of (best non-blank - blank) over the frames
        lg = model.ctc.logits(enc)
        gap = lg[:, 1:VOCAB].max(1).values - lg[:, 0]
        model.ctc.ctc_lo.bias[0] += float(torch.quantile(gap.float().cpu(), 0.9))
        model.ctc.prepare()
    emask = enc_mask.reshape(-1).to(torch.float32).contiguous()
    net, rescore = CTCPrefixBeamSearch(model, BEAM), AttentionRescoring(model, BEAM)

    st = {}

    def timed(name, fn):
        ts = []
        out = None
        for r in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ts.append(e0.elapsed_time(e1))
        st[name] = statistics.median(ts)
        return out

    enc, enc_mask = timed("fbank_encoder_ms", encode)
    logits = timed("ctc_head_ms", lambda: model.ctc.logits(enc))
    timed("greedy_ms", lambda: ops.ctc_greedy_search(logits, b, t2, VOCAB, emask))
    lp, ix = timed("topk_ms", lambda: ops.ctc_topk(logits, VOCAB, BEAM))
    hyp, hyp_len, score, n_hyp = timed("prefix_beam_ms", lambda: ops.ctc_prefix_beam_search(lp, ix, b, t2, BEAM, mask=emask))
    hyp2, lens = hyp.reshape(b * BEAM, t2), hyp_len.reshape(-1)
    ys, ymask = timed("decoder_input_ms", lambda: decoder_input(hyp2, lens, eos, eos))
    l1 = ys.shape[1]
    scores = timed("decoder_ms", lambda: rescore(enc, enc_mask, ys, ymask, BEAM))
    timed("hyp_score_ms", lambda: ops.hyp_score(scores.reshape(b * BEAM * l1, VOCAB), VOCAB, b, BEAM, l1, hyp2, lens, eos,
                                                score.reshape(-1), 0.0, n_hyp))
    # host baseline on the same top-k lists
    lp_h, ix_h, m_h = lp.view(b, t2, BEAM).cpu(), ix.view(b, t2, BEAM).cpu(), emask.view(b, t2).cpu()
    t0 = time.perf_counter()
    agree = 0
    for u in range(a.host_utts):
        keep = m_h[u] != 0
        res = host_prefix_search(lp_h[u][keep].tolist(), ix_h[u][keep].tolist(), BEAM)
        agree += [p for p, _ in res] == [tuple(hyp[u, j, :int(hyp_len[u, j])].tolist()) for j in range(int(n_hyp[u]))]
    host_s = (time.perf_counter() - t0) / max(a.host_utts, 1)
    base = st["fbank_encoder_ms"] + st["ctc_head_ms"]
    search = st["topk_ms"] + st["prefix_beam_ms"]
    rescoring = st["decoder_input_ms"] + st["decoder_ms"] + st["hyp_score_ms"]
    out = {
        "workload": "%d x 10 s synthetic, fbank + hybrid Conformer (12 + 6 blocks, V %d), beam %d" % (BATCH, VOCAB, BEAM),
        "stage_ms": {k: round(v, 3) for k, v in st.items()},
        "utt_per_s": {"ctc_greedy_search": round(BATCH / (base + st["greedy_ms"]) * 1e3, 1),
                      "ctc_prefix_beam_search": round(BATCH / (base + search) * 1e3, 1),
                      "attention_rescoring": round(BATCH / (base + search + rescoring) * 1e3, 1)},
        "beam_plus_rescoring_ms": round(search + rescoring, 3),
        "mean_hyp_len": round(float(hyp_len[:, 0].float().mean()), 1), "decoder_rows": int(b * BEAM * l1),
        "host_prefix_search_s_per_utt": round(host_s, 4), "host_agrees": "%d/%d" % (agree, a.host_utts),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
