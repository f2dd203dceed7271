#!/usr/bin/env python3
"""Decode modes at bench.py's headline workload: 64 x 10 s synthetic waveforms -> fbank -> hybrid Conformer (the shipped shapes:
d 256, 12 encoder blocks, 6 decoder blocks, V = 4233) -> CTC greedy search / CTC prefix beam search (beam 10) / attention rescoring
(beam 10).  Prints per-stage device time (CUDA events, median of --reps), utterances/s of each mode end to end, and the host-side
baseline: the reference's prefix search restated in Python (utils/recognize.py:273-336) on the same top-k lists.

The weights are random, so the CTC head's blank bias is calibrated first: 10 % of the frames are non-blank, about 25 tokens per 10 s
utterance (a trained Chinese model's rate); without it the hypotheses of a random head run to hundreds of tokens.

usage: python tools/decode_bench.py [--reps 10] [--host-utts 4]"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-utts", type=int, default=4)
    a = ap.parse_args()

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
