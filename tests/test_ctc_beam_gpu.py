"""GPU: CTC top-k, the batched CTC prefix beam search, the grouped small attention, the rescoring decoder and score loop, and the
two decode modes of predict() (mindaudio/utils/recognize.py:273-406, models/decoders/decoder_factory.py:195-275).  The searches are
checked against tests/golden/beam_goldens.npz (the reference's own functions, tests/golden/gen_beam_goldens.py)."""
import math
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "beam_goldens.npz"))


def _ref_topk(x64, k):
    lp = x64 - np.log(np.exp(x64 - x64.max(1, keepdims=True)).sum(1, keepdims=True)) - x64.max(1, keepdims=True)
    order = np.stack([np.lexsort((np.arange(lp.shape[1]), -lp[r])) for r in range(lp.shape[0])])
    return lp, order


@pytest.mark.parametrize("V", [11, 4233])
@pytest.mark.parametrize("k", [1, 4, 10, 16])
def test_ctc_topk_matches_log_softmax_sort(V, k):
    import torch

    from mindaudio_amd import ops

    g = torch.Generator().manual_seed(V * 100 + k)
    rows = 1003
    buf = torch.randn(rows, V + 13, generator=g) * 3.0
    buf[::7, 2] = buf[::7, 5] = buf[::7, 9] = buf[::7, :V].max(1).values + 1.0        # planted ties at the top
    buf[1::7, 3] = buf[1::7, 8] = buf[1::7, 1]                                        # ... and further down
    x = buf.cuda()[:, :V]                                                             # strided rows
    if k > V:  # (TopK of more entries than the row has)
        with pytest.raises(ValueError):
            ops.ctc_topk(x, V, k)
        return
    logp, index = ops.ctc_topk(x, V, k)
    lp, order = _ref_topk(buf[:, :V].double().numpy(), k)
    got_v, got_i = logp.cpu().numpy(), index.cpu().numpy()
    want_v = np.take_along_axis(lp, order[:, :k], 1)
    assert np.abs(got_v - want_v).max() <= 1e-5
    top = np.take_along_axis(lp, order[:, :k + 1], 1)
    gaps = np.diff(top, axis=1)
    clean = np.all((gaps == 0) | (np.abs(gaps) > 1e-5), axis=1)                       # distinct values or exact ties
    assert clean.sum() > rows * 0.9
    assert np.array_equal(got_i[clean], order[clean, :k])
    assert np.array_equal(got_i[::7][:, :min(k, 3)], np.tile([2, 5, 9][:min(k, 3)], (len(got_i[::7]), 1)))


def _batch(gold, cases):
    import torch

    beam = gold["pb%d_logp" % cases[0]].shape[1]
    T = max(gold["pb%d_logp" % i].shape[0] for i in cases)
    lp = np.zeros((len(cases), T, beam), np.float32)
    ix = np.zeros((len(cases), T, beam), np.int32)
    mk = np.zeros((len(cases), T), np.float32)
    for u, i in enumerate(cases):
        t = gold["pb%d_logp" % i].shape[0]
        lp[u, :t], ix[u, :t], mk[u, :t] = gold["pb%d_logp" % i], gold["pb%d_index" % i], gold["pb%d_mask" % i]
    f = lambda a: torch.from_numpy(a).cuda().reshape(len(cases) * T, -1).contiguous()  # noqa: E731
    return f(lp), f(ix), torch.from_numpy(mk).cuda().reshape(-1).contiguous(), T, beam


@pytest.mark.parametrize("beam", [1, 4, 10, 16])
def test_prefix_beam_search_matches_the_reference(gold, beam):
    from mindaudio_amd import ops

    cases = [i for i in range(int(gold["pb_n"])) if gold["pb%d_logp" % i].shape[1] == beam]
    assert len(cases) >= 4
    lp, ix, mk, T, _ = _batch(gold, cases)
    hyp, hyp_len, score, n_hyp = ops.ctc_prefix_beam_search(lp, ix, len(cases), T, beam, mask=mk)   # one launch for all of them
    hyp, hyp_len, score, n_hyp = hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy(), n_hyp.cpu().numpy()
    for u, i in enumerate(cases):
        p = "pb%d_" % i
        n = int(gold[p + "n"])
        assert n_hyp[u] == n, i
        assert np.array_equal(hyp_len[u], gold[p + "len"]), i
        t = gold[p + "hyp"].shape[1]
        assert np.array_equal(hyp[u, :, :t], gold[p + "hyp"]) and not hyp[u, :, t:].any(), i
        want = gold[p + "score"]
        assert np.array_equal(np.isneginf(score[u]), np.isneginf(want)), i
        fin = np.isfinite(want)
        assert np.abs(score[u][fin] - want[fin]).max(initial=0.0) <= 1e-9, i


def test_beam_one_is_greedy():
    import torch

    from mindaudio_amd import ops

    torch.manual_seed(5)
    b, t, v = 6, 61, 30
    logits = (torch.randn(b * t, v) * 2.0).cuda()
    logits[:, 0] += 1.5
    mask = torch.ones(b, t)
    for u, n in enumerate([61, 60, 40, 33, 7, 1]):
        mask[u, n:] = 0                                       # tail masks, as the encoder gives
    mask = mask.cuda().reshape(-1).contiguous()
    _, _, g_hyp, g_len = ops.ctc_greedy_search(logits, b, t, v, mask)
    lp, ix = ops.ctc_topk(logits, v, 1)
    hyp, hyp_len, _, n_hyp = ops.ctc_prefix_beam_search(lp, ix, b, t, 1, mask=mask)
    assert n_hyp.cpu().tolist() == [1] * b
    assert torch.equal(hyp_len[:, 0].cpu(), g_len.cpu())
    assert torch.equal(hyp[:, 0].cpu(), g_hyp.cpu())


@pytest.mark.parametrize("lq,lk", [(12, 40), (45, 319), (9, 321), (33, 500)])
def test_grouped_small_attention_is_the_repeated_one(lq, lk):
    import torch

    from mindaudio_amd.train import kernels as K

    torch.manual_seed(lq + lk)
    bm, g, d = 3, 4, 256
    q = torch.randn(bm * g * lq, d).cuda().to(torch.bfloat16)
    kv = torch.randn(bm * lk, 2 * d).cuda().to(torch.bfloat16)
    mask = torch.ones(bm, lk)
    mask[1, lk - 7:] = 0
    mask[2, lk // 3:] = 0
    mask = mask.cuda()
    ctx_g, probs_g = K.mha_small_fwd_grouped(q, kv[:, :d], kv[:, d:], mask, 1, bm * g, lq, lk, 1.0 / 64, g)
    kvr = kv.view(bm, lk, 2 * d).repeat_interleave(g, 0).reshape(bm * g * lk, 2 * d)
    ctx_r, probs_r = K.mha_small_fwd(q, kvr[:, :d], kvr[:, d:], mask.repeat_interleave(g, 0).contiguous(), 1, bm * g, lq, lk,
                                     1.0 / 64)
    assert torch.equal(ctx_g.view(torch.int16), ctx_r.view(torch.int16))
    assert torch.equal(probs_g, probs_r)


def _hybrid(vocab, d=256, heads=4, blocks=2, dblocks=2, seed=7):
    import torch

    from mindaudio_amd.conformer.asr_model import create_asr_model

    torch.manual_seed(seed)
    model = create_asr_model(80, vocab, dict(output_size=d, attention_heads=heads, linear_units=512, num_blocks=blocks),
                             ctc_weight=0.3, decoder_conf=dict(attention_heads=heads, linear_units=512, num_blocks=dblocks))
    return model.cuda().eval()


def test_score_hypotheses_is_forward_on_repeated_memory_and_matches_the_oracle():
    import torch

    from mindaudio_amd.conformer.asr_model import decoder_input
    from oracle import conformer_oracle as C

    torch.manual_seed(11)
    vocab, d, bm, g, t2 = 97, 256, 3, 5, 71
    ref_dec = C.TransformerDecoder(vocab, d, 4, 512, 2, 0.0, 0.0).eval()
    model = _hybrid(vocab)
    missing, unexpected = model.decoder.load_state_dict(ref_dec.state_dict(), strict=False)
    assert not missing and not unexpected
    mem = torch.randn(bm, t2, d)
    mmask = torch.ones(bm, 1, t2)
    mmask[1, 0, 50:] = 0
    mmask[2, 0, 20:] = 0
    lens = torch.randint(0, 14, (bm * g,), dtype=torch.int32)
    lens[3] = 0
    hyp = torch.randint(1, vocab - 1, (bm * g, 20), dtype=torch.int32)
    ys, masks = decoder_input(hyp, lens, vocab - 1, vocab - 1)
    got = model.decoder.score_hypotheses(mem.cuda(), mmask.cuda(), ys.cuda(), masks.cuda(), g)
    rep, _ = model.decoder(mem.repeat_interleave(g, 0).cuda(), mmask.repeat_interleave(g, 0).cuda(), ys.cuda(), masks.cuda())
    assert got.shape == rep.shape == (bm * g, ys.shape[1], vocab)
    assert float((got - rep).abs().max()) <= 1e-6
    with torch.no_grad():
        want = torch.log_softmax(ref_dec(mem.repeat_interleave(g, 0), mmask.repeat_interleave(g, 0), ys.long(), masks), -1)
    lsm = torch.log_softmax(got.cpu(), -1)
    valid = torch.arange(ys.shape[1])[None] <= lens[:, None].long()
    err = (lsm - want)[valid]
    assert float(err.pow(2).mean().sqrt() / want[valid].pow(2).mean().sqrt()) <= 2e-2


def test_hyp_score_matches_the_reference_rescoring(gold):
    import torch

    from mindaudio_amd import ops

    for i in range(int(gold["rs_n"])):
        p = "rs%d_" % i
        logits = torch.from_numpy(gold[p + "logits"])
        beam, l31, v = logits.shape
        buf = torch.zeros(beam * l31, v + 64 - v % 64)
        buf[:, :v] = logits.reshape(-1, v)
        x = buf.cuda()[:, :v]
        hyp = torch.from_numpy(np.pad(gold[p + "hyp"], ((0, 0), (0, l31)))).cuda()
        lens = torch.from_numpy(gold[p + "len"]).cuda()
        ctc = torch.from_numpy(gold[p + "score"]).cuda()
        scores, best, best_score = ops.hyp_score(x, v, 1, beam, l31, hyp, lens, int(gold[p + "eos"]), ctc, float(gold[p + "ctc_weight"]))
        assert int(best[0]) == int(gold[p + "best"]), i
        assert abs(float(best_score[0]) - float(gold[p + "best_score"])) <= 1e-5, i
    # the prefix search feeding it, batched over the rescoring cases of one beam size
    for beam in (4, 10):
        cases = [i for i in range(int(gold["rs_n"])) if gold["rs%d_logits" % i].shape[0] == beam]
        for i in cases:
            p = "rs%d_" % i
            lp = torch.from_numpy(gold[p + "logp"]).cuda().contiguous()
            ix = torch.from_numpy(gold[p + "index"]).cuda().contiguous()
            mk = torch.from_numpy(gold[p + "mask"]).cuda().contiguous()
            hyp, hyp_len, score, n = ops.ctc_prefix_beam_search(lp, ix, 1, lp.shape[0], beam, mask=mk)
            assert np.array_equal(hyp[0].cpu().numpy(), gold[p + "hyp"]) and np.abs(score[0].cpu().numpy() - gold[p + "score"]).max() <= 1e-9


def _host_prefix_search(lp_row, idx_row, frames, beam):
    """recognize.py:273-336 restated for identical frames (test oracle)."""
    def log_add(args):
        if all(a == -math.inf for a in args):
            return -math.inf
        m = max(args)
        return m + math.log(sum(math.exp(a - m) for a in args))

    cur = [((), (0.0, -math.inf))]
    for _ in range(frames):
        nxt = {}
        for ps, s in zip(lp_row, idx_row):
            for prefix, (pb, pnb) in cur:
                last = prefix[-1] if prefix else None
                if s == 0:
                    a, bb = nxt.get(prefix, (-math.inf, -math.inf))
                    nxt[prefix] = (log_add([a, pb + ps, pnb + ps]), bb)
                elif s == last:
                    a, bb = nxt.get(prefix, (-math.inf, -math.inf))
                    nxt[prefix] = (a, log_add([bb, pnb + ps]))
                    a, bb = nxt.get(prefix + (s,), (-math.inf, -math.inf))
                    nxt[prefix + (s,)] = (a, log_add([bb, pb + ps]))
                else:
                    a, bb = nxt.get(prefix + (s,), (-math.inf, -math.inf))
                    nxt[prefix + (s,)] = (a, log_add([bb, pb + ps, pnb + ps]))
        cur = sorted(nxt.items(), key=lambda kv: log_add(list(kv[1])), reverse=True)[:beam]
    return [(p, log_add(list(v))) for p, v in cur]


def test_predict_beam_modes_on_a_manifest(tmp_path):
    """predict() with decode_mode ctc_prefix_beam_search / attention_rescoring on a small hybrid model whose CTC head and decoder output
    layer have zero weights: every frame's CTC distribution is softmax(ctc bias) (blank and token 3 only, the rest ~e-10) and every
    decoder position's is softmax(output bias) (token 3 and eos equal).  The CTC first-best is the length of 3s the frames favour; the
    rescoring (ctc_weight 0) keeps the SHORTEST hypothesis of the beam, a different one.  Also through a checkpoint file."""
    import wave

    import torch
    import yaml

    from mindaudio_amd.conformer import predict as P
    from mindaudio_amd.conformer import train as T
    from mindaudio_amd.conformer.dataset import compute_fbank_feats_batch
    from mindaudio_amd.data.io import read
    from mindaudio_amd.utils.ckpt import to_reference_names, write_mindspore_ckpt
    from test_conformer_train_script import YAML

    src = os.path.join(HERE, "golden", "BAC009S0002W0122.wav")
    with wave.open(src, "rb") as w:
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    syms = ["<blank>", "<unk>", "a", "b", "c", "d", "e", "<sos/eos>"]
    (tmp_path / "lang_char.txt").write_text("".join("%s %d\n" % (s, i + 2) for i, s in enumerate(syms)))
    rows = ["id,duration,wav,transcript"]
    for i, (n, text) in enumerate(((30000, "abc"), (52000, "dd"), (90000, "cab"))):
        p = str(tmp_path / ("utt%d.wav" % i))
        with wave.open(p, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.resize(pcm, n).tobytes())
        rows.append("%d,%.2f,%s,%s" % (i, n / 16000.0, p, text))
    (tmp_path / "test.csv").write_text("\n".join(rows) + "\n")
    cfg = yaml.safe_load(YAML)
    cfg.update(test_data=str(tmp_path / "test.csv"), dict=str(tmp_path / "lang_char.txt"), exp_name=str(tmp_path / "exp"),
               decode_ckpt="avg.ckpt", beam_size=4, ctc_weight=0.0)
    sos, eos, vocab, char_dict = P.load_language_dict(cfg["dict"])
    torch.manual_seed(3)
    model = T.build_model(cfg, 80, vocab, torch.device("cuda"))
    with torch.no_grad():
        model.ctc.ctc_lo.weight.zero_()
        model.ctc.ctc_lo.bias.fill_(-20.0)
        model.ctc.ctc_lo.bias[0] = 2.0
        model.ctc.ctc_lo.bias[3] = 1.5
        model.decoder.output_layer.weight.zero_()
        model.decoder.output_layer.bias.fill_(-20.0)
        model.decoder.output_layer.bias[3] = 0.0
        model.decoder.output_layer.bias[eos] = 0.0
    # the expected hypotheses: the CTC top-4 of every frame (float32 log_softmax, as the kernel), the number of valid encoder frames
    cb = model.ctc.ctc_lo.bias.detach().cpu().float()
    lp32 = torch.log_softmax(cb, 0)
    order = sorted(range(vocab), key=lambda j: (-float(lp32[j]), j))[:4]
    lp_row, idx_row = [float(lp32[j]) for j in order], order
    fe = cfg["collate_conf"]["feature_extraction_conf"]
    buckets = [int(v) for v in str(cfg["dataset_conf"]["frame_bucket_limit"]).split(",")]
    want_beam, want_res = [], []
    dl = torch.log_softmax(model.decoder.output_layer.bias.detach().cpu().double(), 0)
    for uttid, path, frames, _ in P.predict_samples(cfg["test_data"], cfg["dict"], cfg["dataset_conf"]):
        wav, sr = read(path)
        _, nfr = compute_fbank_feats_batch((np.asarray(wav, np.float32) * (1 << 15))[None], [len(wav)], sample_rate=sr,
                                           frame_len=int(fe["frame_length"]), frame_shift=int(fe["frame_shift"]),
                                           mel_bin=int(fe["mel_bins"]))
        n = int(nfr[0])
        pad = max(P.bucket_length(frames, buckets), n)
        m = torch.zeros(1, 1, pad)
        m[0, 0, :n] = 1
        nv = int(m[:, :, :-2:2][:, :, :-2:2].sum())
        hyps = _host_prefix_search(lp_row, idx_row, nv, 4)
        assert len(hyps) == 4 and all(len(h[0]) > 0 for h in hyps)
        res = [sum(float(dl[w]) for w in h[0]) + float(dl[eos]) for h in hyps]
        best = max(range(4), key=lambda j: (res[j], -j))
        assert hyps[best][0] != hyps[0][0]                       # the rescoring changes the answer
        text = lambda h: "".join(str(c) for c in P.ids_to_text(list(h), eos, char_dict))  # noqa: E731
        want_beam.append("%s %s" % (uttid, text(hyps[0][0])))
        want_res.append("%s %s" % (uttid, text(hyps[best][0])))
    assert want_beam != want_res
    for mode, want in (("ctc_prefix_beam_search", want_beam), ("attention_rescoring", want_res)):
        lines = []
        mean, results = P.predict(dict(cfg, decode_mode=mode), log=lines.append, model=model)
        got = (tmp_path / "exp" / ("test_" + mode) / "result.txt").read_text().splitlines()
        assert got == want, (mode, got, want)
        assert sum(ln.startswith("cer : ") for ln in lines) == 3 and lines[-1].startswith("cer_average : ")
    os.makedirs(str(tmp_path / "exp" / "model"), exist_ok=True)
    write_mindspore_ckpt(str(tmp_path / "exp" / "model" / "avg.ckpt"), to_reference_names(model.state_dict()))
    os.remove(str(tmp_path / "exp" / "test_attention_rescoring" / "result.txt"))
    _, results2 = P.predict(dict(cfg, decode_mode="attention_rescoring"), log=lambda _l: None)
    assert (tmp_path / "exp" / "test_attention_rescoring" / "result.txt").read_text().splitlines() == want_res
    with pytest.raises(NotImplementedError):
        P.predict(dict(cfg, decode_mode="attention"), log=lambda _l: None, model=model)


def test_attention_rescoring_batched_is_one_at_a_time():
    import torch

    from mindaudio_amd.conformer.asr_model import AttentionRescoring, CTCPrefixBeamSearch, attention_rescoring, ctc_prefix_beam_search

    vocab, beam = 57, 6
    model = _hybrid(vocab, seed=19)
    with torch.no_grad():
        model.ctc.ctc_lo.weight.mul_(4.0)               # a peakier CTC head than the random initialisation gives
        model.ctc.ctc_lo.bias[0] = 2.0
    net, rescore = CTCPrefixBeamSearch(model, beam), AttentionRescoring(model, beam)
    torch.manual_seed(2)
    tlen = 300
    lens = [300, 271, 250, 199, 160, 97, 40]
    xs = torch.randn(len(lens), tlen, 80).cuda()
    masks = torch.zeros(len(lens), 1, tlen).cuda()
    for u, n in enumerate(lens):
        masks[u, 0, :n] = 1
    eos = vocab - 1
    hyps, scores = attention_rescoring(net, rescore, xs, masks, None, eos, eos, beam, 0.3)
    beams, _, _ = ctc_prefix_beam_search(net, xs, masks, beam)
    for u in range(len(lens)):
        h1, s1 = attention_rescoring(net, rescore, xs[u:u + 1], masks[u:u + 1], None, eos, eos, beam, 0.3)
        b1, _, _ = ctc_prefix_beam_search(net, xs[u:u + 1], masks[u:u + 1], beam)
        assert h1[0] == hyps[u], u
        assert abs(s1[0] - scores[u]) <= 1e-4 * abs(scores[u]), u  # (the encoder's GEMMs over 1 or 7 utterances: last bits)
        assert [h for h, _ in b1[0]] == [h for h, _ in beams[u]], u
