"""GPU: the autoregressive `attention` decode mode - ma_decoder_self_attn_step_bf16 (exact one-hot cases, guard bands, a random case
against float64, refusals), ma_attn_beam_step_f32 / ma_attn_beam_best_f32 on every recorded step of the reference's own search,
recognize() driven by the recorded logits, TransformerDecoder.step against the float64 restatement, the search end to end on small
seeded models, and predict() with decode_mode attention + full_graph.  The cases, restatements and comparators are those of
tests/attn_decode_cases.py, proven on the CPU by tests/test_attn_decode_cases_cpu.py."""
import os

import numpy as np
import pytest

import attn_decode_cases as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.0


@pytest.fixture(scope="module")
def gold():
    return C.goldens()


def _dev(x, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _guarded(shape, dtype, guard):
    """A sentinel-filled tensor of `shape` between two sentinel-filled guard bands of `guard` elements: (view, whole buffer)."""
    import torch

    n = int(np.prod(shape))
    whole = torch.full((guard + n + guard,), SENTINEL, dtype=dtype, device="cuda")
    return whole[guard:guard + n].view(*shape), whole


def _bands_untouched(whole, guard):
    return bool((whole[:guard] == SENTINEL).all()) and bool((whole[-guard:] == SENTINEL).all())


# ---- 1. ma_decoder_self_attn_step_bf16 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,lmax", C.STEP_SHAPES)
def test_self_attn_step_exact_positions_parents_and_guard_bands(R, lmax):
    import torch

    from mindaudio_amd import ops

    bf = torch.bfloat16
    oh = C.OneHot(R, lmax)
    d, guard = oh.d, 2 * oh.d
    k_in, v_in, k_new, v_new = (_dev(x, bf) for x in (oh.k_in, oh.v_in, oh.k_new, oh.v_new))
    for t in C.step_ts(lmax):
        for shift in range(t + 1):
            qkv, parent, want_ctx, want_k, want_v = oh.case(t, shift)
            (k_out, k_whole), (v_out, v_whole), (ctx, c_whole) = (_guarded(s, bf, guard) for s in ((R, lmax, d), (R, lmax, d), (R, d)))
            par = _dev(parent)
            got = ops.decoder_self_attn_step(_dev(qkv, bf), k_in, v_in, t, k_out, v_out, oh.heads, 1.0 / 64, parent=par, ctx=ctx)
            assert got is ctx
            C.check_ctx_exact(ctx.float().cpu().numpy(), want_ctx)
            # the cache copy and the appended row, bit for bit; positions above t and the guard bands untouched
            p64 = par.long()
            assert torch.equal(k_out[:, :t], k_in[p64, :t]) and torch.equal(v_out[:, :t], v_in[p64, :t]), (t, shift)
            assert torch.equal(k_out[:, t], k_new[:, t]) and torch.equal(v_out[:, t], v_new[:, t]), (t, shift)
            assert bool((k_out[:, t + 1:] == SENTINEL).all()) and bool((v_out[:, t + 1:] == SENTINEL).all()), (t, shift)
            assert all(_bands_untouched(w, guard) for w in (k_whole, v_whole, c_whole)), (t, shift)
            if shift in (0, t):
                C.check_cache(k_out.float().cpu().numpy(), v_out.float().cpu().numpy(), want_k, want_v, t)


def test_self_attn_step_parent_duplicates_permutation_and_null():
    import torch

    from mindaudio_amd import ops

    bf = torch.bfloat16
    R, lmax, t = 10, 70, 33
    oh = C.OneHot(R, lmax)
    k_in, v_in = _dev(oh.k_in, bf), _dev(oh.v_in, bf)
    rng = np.random.RandomState(4)
    target = rng.randint(0, t + 1, size=R)
    for parent in (np.array([3, 3, 3, 0, 0, 9, 9, 9, 9, 1], np.int32), rng.permutation(R).astype(np.int32), None):
        par = np.arange(R) if parent is None else parent
        qkv = np.concatenate([oh.q_pat[target], oh.k_new[:, t], oh.v_new[:, t]], 1)
        k_out, v_out = torch.zeros_like(k_in), torch.zeros_like(v_in)
        ctx = ops.decoder_self_attn_step(_dev(qkv, bf), k_in, v_in, t, k_out, v_out, oh.heads, 1.0 / 64,
                                         parent=None if parent is None else _dev(parent))
        want_k, want_v = C.cache_update(oh.k_in, oh.v_in, oh.k_new[:, t], oh.v_new[:, t], par, t)
        C.check_cache(k_out.float().cpu().numpy(), v_out.float().cpu().numpy(), want_k, want_v, t)
        C.check_ctx_exact(ctx.float().cpu().numpy(), want_v[np.arange(R), target])


@pytest.mark.parametrize("R,lmax", C.STEP_SHAPES)
def test_self_attn_step_random_against_float64_and_twice_the_same_bits(R, lmax):
    import torch

    from mindaudio_amd import ops

    bf = torch.bfloat16
    rng = np.random.RandomState(R * 100 + lmax)
    d = C.HEADS * 64
    k_in, v_in = C.bf16(rng.randn(R, lmax, d)), C.bf16(2.0 * rng.randn(R, lmax, d))
    for t in C.step_ts(lmax):
        qkv = C.bf16(rng.randn(R, 3 * d) * np.array([4.0] * d + [1.0] * d + [2.0] * d))  # scores with a spread of a few units
        parent = rng.randint(0, R, size=R).astype(np.int32)
        want_ctx, want_k, want_v = C.self_attn_step(qkv, k_in, v_in, parent, t, C.HEADS, 1.0 / 64)
        runs = []
        for _ in range(2):
            k_out, v_out = torch.zeros((R, lmax, d), dtype=bf, device="cuda"), torch.zeros((R, lmax, d), dtype=bf, device="cuda")
            ctx = ops.decoder_self_attn_step(_dev(qkv.astype(np.float32), bf), _dev(k_in.astype(np.float32), bf),
                                             _dev(v_in.astype(np.float32), bf), t, k_out, v_out, C.HEADS, 1.0 / 64, parent=_dev(parent))
            runs.append((ctx, k_out, v_out))
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        ctx, k_out, v_out = runs[0]
        C.check_cache(k_out.float().cpu().numpy(), v_out.float().cpu().numpy(), want_k, want_v, t)
        C.check_ctx_close(ctx.float().cpu().numpy(), want_ctx, want_v[:, :t + 1])


def test_self_attn_step_refusals():
    import torch

    from mindaudio_amd import _host, _lib, ops

    bf = torch.bfloat16
    R, lmax, d = 4, 9, 256
    qkv = torch.zeros((R, 3 * d), dtype=bf, device="cuda")
    a, b, c, e = (torch.zeros((R, lmax, d), dtype=bf, device="cuda") for _ in range(4))
    ops.decoder_self_attn_step(qkv, a, b, 0, c, e, 4, 1.0 / 64)
    with pytest.raises(ValueError):
        ops.decoder_self_attn_step(qkv, a, b, lmax, c, e, 4, 1.0 / 64)              # t >= Lmax
    for k_out, v_out in ((a, e), (c, b), (c, c), (b, e)):                            # an in buffer is an out buffer
        with pytest.raises(ValueError):
            ops.decoder_self_attn_step(qkv, a, b, 3, k_out, v_out, 4, 1.0 / 64)
    with pytest.raises(NotImplementedError):
        ops.decoder_self_attn_step(qkv, a, b, 0, c, e, 2, 1.0 / 128)                 # d_k 128
    lib, p, s = _lib.load(), _host.ptr, _host.current_stream_ptr()
    ctx = torch.zeros((R, d), dtype=bf, device="cuda")
    call = lambda rows, heads, dk, dd: lib.ma_decoder_self_attn_step_bf16(p(qkv), 3 * d, p(a), p(b), None, rows, lmax, 0, heads, dk, dd,  # noqa: E731
                                                                          1.0 / 64, p(ctx), d, p(c), p(e), s)
    assert call(0, 4, 64, d) == _lib.MA_ERR_INVALID_ARG                               # R == 0
    assert call(R, 4, 64, 192) == _lib.MA_ERR_UNSUPPORTED                             # d != heads * 64
    assert call(R, 4, 32, 128) == _lib.MA_ERR_UNSUPPORTED                             # d_k != 64
    assert call(R, 4, 64, d) == _lib.MA_OK
    torch.cuda.synchronize()


# ---- 2. ma_attn_beam_step_f32 / ma_attn_beam_best_f32 --------------------------------------------------------------------------------
def test_beam_step_every_recorded_step(gold):
    import torch

    from mindaudio_amd import ops

    for name in C.golden_names(gold):
        eos = int(gold[name + "_eos"])
        for s in range(int(gold[name + "_steps"])):
            ins, want, n, maxlen = C.golden_step(gold, name, s)
            length = torch.full((1,), s, dtype=torch.int32, device="cuda")
            done = torch.zeros(1, dtype=torch.int32, device="cuda")
            out = ops.attn_beam_step(_dev(ins["tk_logp"]), _dev(ins["tk_index"]), _dev(ins["scores_in"]), _dev(ins["end_in"]),
                                     _dev(ins["tokens_in"]), length, done, eos, maxlen - 1)
            got = [x.cpu().numpy() for x in out] + [int(length[0]), int(done[0])]
            C.check_beam(got, want)
        # the final pick
        p = name + "_"
        hyp, ln, score = ops.attn_beam_best(_dev(gold[p + "scores_out"][-1]), _dev(gold[p + "tokens_out"][-1]),
                                            torch.full((1,), int(gold[p + "steps"]), dtype=torch.int32, device="cuda"), n)
        assert np.array_equal(hyp.cpu().numpy()[0], gold[p + "best_hyps"]) and int(ln[0]) == int(gold[p + "steps"])
        assert score.cpu().numpy()[0] == gold[p + "best_score"]


def test_beam_best_first_of_equal_maxima_and_infinities():
    import torch

    from mindaudio_amd import ops

    scores = np.array([[-2.0, -1.0, -1.0, -3.0], [-np.inf, -np.inf, -np.inf, -np.inf], [-5.0, -np.inf, 0.0, 0.0]], np.float32)
    tokens = np.arange(3 * 4 * 5, dtype=np.int32).reshape(12, 5)
    hyp, ln, best = ops.attn_beam_best(_dev(scores.reshape(-1)), _dev(tokens), _dev(np.array([4, 2, 3], np.int32)), 4)
    assert np.array_equal(hyp.cpu().numpy(), tokens.reshape(3, 4, 5)[[0, 1, 2], [1, 0, 2], 1:])
    assert ln.cpu().tolist() == [4, 2, 3] and np.array_equal(best.cpu().numpy(), np.array([-1.0, -np.inf, 0.0], np.float32))


def test_beam_step_batch_of_three_is_three_single_calls(gold):
    """Three golden cases of beam 4 and one eos as one batch, token rows padded to the common width (that of the case the length
    limit ends; the other two end by eos): every utterance gets its own one-utterance result at every step, and the early finishers
    stay frozen (scores, flags, tokens, length unchanged, parent the identity)."""
    import torch

    from mindaudio_amd import ops

    names = ("beam4", "all_finish_step1", "length_limit")
    n, W = 4, int(gold["length_limit_maxlen"])
    eos = int(gold["beam4_eos"])
    assert all(int(gold[nm + "_beam"]) == n and int(gold[nm + "_eos"]) == eos and int(gold[nm + "_maxlen"]) <= W for nm in names)
    steps = [int(gold[nm + "_steps"]) for nm in names]
    assert steps[2] == W - 1 and steps[0] < int(gold["beam4_maxlen"]) - 1 and steps[1] == 2
    sc = _dev(np.concatenate([gold[nm + "_scores_in"][0] for nm in names]))
    en = _dev(np.concatenate([gold[nm + "_end_in"][0] for nm in names]))
    tok0 = np.zeros((3 * n, W), np.int32)
    for u, nm in enumerate(names):
        tok0[u * n:(u + 1) * n, :int(gold[nm + "_maxlen"])] = gold[nm + "_tokens_in"][0]
    tk = _dev(tok0)
    length = torch.zeros(3, dtype=torch.int32, device="cuda")
    done = torch.zeros(3, dtype=torch.int32, device="cuda")
    for s in range(max(steps)):
        lp, ix = np.zeros((3 * n, n), np.float32), np.zeros((3 * n, n), np.int32)
        for u, nm in enumerate(names):  # (a frozen utterance is handed its last step's lists again: they must not matter)
            k = min(s, steps[u] - 1)
            lp[u * n:(u + 1) * n], ix[u * n:(u + 1) * n] = gold[nm + "_tk_logp"][k], gold[nm + "_tk_index"][k]
        before = (sc.clone(), en.clone(), tk.clone())
        sc, en, tk, parent, pred = ops.attn_beam_step(_dev(lp), _dev(ix), sc, en, tk, length, done, eos, W - 1)
        for u, nm in enumerate(names):
            rows = slice(u * n, (u + 1) * n)
            wm = int(gold[nm + "_maxlen"])
            if s < steps[u]:
                want = (gold[nm + "_scores_out"][s], gold[nm + "_end_out"][s], gold[nm + "_tokens_out"][s], gold[nm + "_parent"][s] + u * n,
                        gold[nm + "_pred"][s], s + 1, int(s == steps[u] - 1))
                got = (sc[rows].cpu().numpy(), en[rows].cpu().numpy(), tk[rows, :wm].cpu().numpy(), parent[rows].cpu().numpy(),
                       pred[rows].cpu().numpy(), int(length[u]), int(done[u]))
                C.check_beam(got, want)
                assert not tk[rows, wm:].any()
            else:
                assert torch.equal(sc[rows], before[0][rows]) and torch.equal(en[rows], before[1][rows])
                assert torch.equal(tk[rows], before[2][rows]) and int(length[u]) == steps[u] and int(done[u]) == 1
                assert parent[rows].cpu().tolist() == list(range(u * n, (u + 1) * n))


# ---- 3. recognize() on the recorded logits ---------------------------------------------------------------------------------------------
class _Recorded:
    """A logits source that replays a golden case (steps issued past the recorded ones get the last step's logits again)."""

    def __init__(self, gold, name):
        self.logits = [_dev(x) for x in gold[name + "_logits"]]
        self.maxlen, self.beam_size, self.calls = int(gold[name + "_maxlen"]), int(gold[name + "_beam"]), 0

    def begin(self, xs_pad, xs_masks, xs_lengths=None):
        def step(tokens, t, parent=None):
            self.calls += 1
            return self.logits[min(t, len(self.logits) - 1)]

        return self.maxlen, step


@pytest.mark.parametrize("chunk", (1, 3, 8))
def test_recognize_on_recorded_logits_equals_the_reference(gold, chunk):
    import torch

    from mindaudio_amd.conformer.asr_model import recognize

    for name in C.golden_names(gold):
        p = name + "_"
        n, sos, eos, steps = int(gold[p + "beam"]), int(gold[p + "sos"]), int(gold[p + "eos"]), int(gold[p + "steps"])
        src = _Recorded(gold, name)
        hyps, scores = recognize(src, torch.zeros(1, 8, 2, device="cuda"), torch.ones(1, 1, 8, device="cuda"), np.array([sos], np.int32),
                                 np.zeros((1, 1), np.int32), np.array([0.0] + [-np.inf] * (n - 1), np.float32), np.zeros(n, np.float32),
                                 n, eos, None, True, chunk)
        assert hyps.shape == (1, src.maxlen - 1) and np.array_equal(hyps[0], gold[p + "best_hyps"]), (name, hyps[0])
        assert scores.shape == (1,) and scores[0] == gold[p + "best_score"], name
        # whole chunks are issued (steps past `done` among them), never more than maxlen - 1 steps
        assert src.calls == min(-(-steps // chunk) * chunk, src.maxlen - 1), (name, src.calls)


# ---- 4. TransformerDecoder.step against the float64 restatement ------------------------------------------------------------------------
def _decoder(sd, vocab):
    import torch

    from mindaudio_amd.models.decoder import TransformerDecoder

    dec = TransformerDecoder(vocab, C.D, attention_heads=C.HEADS, linear_units=C.UNITS, num_blocks=C.BLOCKS)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return dec.cuda().eval()


def test_decoder_step_and_forward_meet_the_same_yardstick():
    """The logits of steps 1, 2, 33 and maxlen - 1 on random weights, random tokens and random beam reorders: TransformerDecoder.step
    (KV cache) and TransformerDecoder.forward on the full prefix are both held to 2 S against the float64 restatement, S being what
    the restatement gives with bf16 rounding at the device's rounding points."""
    import torch

    vocab, rows, group, frames = C.STEP_MODEL
    rng = np.random.RandomState(17)
    sd = C.random_weights(23, vocab)
    memory = rng.randn(rows // group, frames, C.D).astype(np.float32)
    mask = np.ones((rows // group, frames), bool)
    mask[1, frames - 5:] = False
    exact, rounded = C.Decoder(sd), C.Decoder(sd, rnd=C.bf16)
    caches = [m.init_cache(memory.astype(np.float64), mask, group, frames) for m in (exact, rounded)]
    dec = _decoder(sd, vocab)
    mem_d, mask_d = _dev(memory), _dev(mask.astype(np.float32)[:, None, :])
    cache = dec.init_cache(mem_d, mask_d, group, frames)
    ids = np.zeros((rows, frames), np.int64)
    ids[:, 0] = vocab - 1
    parent, checked = None, 0
    for t in range(frames - 1):
        want, rnd = (m.step(c, ids[:, t], t, parent) for m, c in zip((exact, rounded), caches))
        got = dec.step(cache, _dev(ids[:, t].astype(np.int32)), t, None if parent is None else _dev(parent.astype(np.int32)))
        if t + 1 in C.STEP_MODEL_TS:
            S = C.relrms(rnd, want)
            e_step = C.relrms(got.cpu().numpy(), want)
            sub = torch.tril(torch.ones(t + 1, t + 1, device="cuda"))[None].repeat(rows, 1, 1)
            full, _ = dec.forward(mem_d.repeat_interleave(group, 0), mask_d.repeat_interleave(group, 0), _dev(ids[:, :t + 1].astype(np.int32)),
                                  sub)
            e_full = C.relrms(full[:, t].cpu().numpy(), want)
            print("step %d: S %.3e, step %.3e, forward %.3e" % (t + 1, S, e_step, e_full))
            assert 1e-4 < S < 3e-2 and e_step <= 2 * S and e_full <= 2 * S, (t + 1, S, e_step, e_full)
            checked += 1
        parent = np.concatenate([u * group + rng.randint(0, group, size=group) for u in range(rows // group)])
        ids = ids[parent]
        ids[:, t + 1] = rng.randint(0, vocab, size=rows)
    assert checked == len(C.STEP_MODEL_TS)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
class _Backbone:
    """An ASR model whose encoder returns a prepared output: the search is compared on the decoder alone."""

    def __init__(self, decoder, memory, mask):
        self.decoder, self.memory, self.mask = decoder, memory, mask

    def encoder(self, xs_pad, masks, chunk_masks):
        return self.memory, self.mask


@pytest.mark.parametrize("case", C.E2E, ids=lambda c: "seed%d-beam%d" % (c[0], c[2]))
def test_recognize_end_to_end_equals_the_float64_search(case):
    import torch

    from mindaudio_amd.conformer.asr_model import Attention, recognize

    seed, vocab, beam, frames = case
    sd, memory, mask, ref = C.e2e_reference(*case)
    if ref["min_gap"] <= C.GUARD:
        return  # not kept: a decision closer than the guard (tests/test_attn_decode_cases_cpu.py holds the count of kept cases)
    net = Attention(_Backbone(_decoder(sd, vocab), _dev(memory), _dev(mask.astype(np.float32)[:, None, :])), beam, vocab - 1)
    hyps, scores = recognize(net, torch.zeros(1, 4 * frames + 8, 2, device="cuda"), torch.ones(1, 1, 4 * frames + 8, device="cuda"),
                             np.array([vocab - 1], np.int32), np.zeros((1, 1), np.int32),
                             np.array([0.0] + [-np.inf] * (beam - 1), np.float32), np.zeros(beam, np.float32), beam, vocab - 1)
    assert np.array_equal(hyps[0], ref["best_hyps"]), (hyps[0].tolist(), ref["best_hyps"].tolist())
    assert abs(float(scores[0]) - float(ref["best_score"])) <= C.GUARD


# ---- 6. predict() ----------------------------------------------------------------------------------------------------------------------
def test_predict_attention_mode_on_a_manifest(tmp_path):
    """predict() with decode_mode attention + full_graph on the small hybrid model of the rescoring test, whose decoder output layer
    has zero weights and a bias: every step's distribution is softmax(bias) whatever the prefix - token 3 far ahead, then eos, the
    rest ~e-30.  With beam 2 the search keeps "3 3 3 ..." and the hypothesis that took eos at once; the run of 3s loses ~5e-5 per
    step and stays ahead of log p(eos) = -10 up to the length limit, so the text is maxlen - 1 times the symbol of token 3.  The
    expected rows are the float64 search's on the same logits at each utterance's encoder frame count.  Also through a checkpoint
    file, and the host-stepped form refuses."""
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
               decode_ckpt="avg.ckpt", beam_size=2, decode_mode="attention", full_graph=True)
    sos, eos, vocab, char_dict = P.load_language_dict(cfg["dict"])
    torch.manual_seed(3)
    model = T.build_model(cfg, 80, vocab, torch.device("cuda"))
    with torch.no_grad():
        model.decoder.output_layer.weight.zero_()
        model.decoder.output_layer.bias.fill_(-20.0)
        model.decoder.output_layer.bias[3] = 10.0
        model.decoder.output_layer.bias[eos] = 0.0
    bias = model.decoder.output_layer.bias.detach().cpu().double().numpy()
    fe = cfg["collate_conf"]["feature_extraction_conf"]
    buckets = [int(v) for v in str(cfg["dataset_conf"]["frame_bucket_limit"]).split(",")]
    want = []
    for uttid, path, frames, _ in P.predict_samples(cfg["test_data"], cfg["dict"], cfg["dataset_conf"]):
        wav, sr = read(path)
        _, nfr = compute_fbank_feats_batch((np.asarray(wav, np.float32) * (1 << 15))[None], [len(wav)], sample_rate=sr,
                                           frame_len=int(fe["frame_length"]), frame_shift=int(fe["frame_shift"]),
                                           mel_bin=int(fe["mel_bins"]))
        pad = max(P.bucket_length(frames, buckets), int(nfr[0]))
        maxlen = torch.zeros(1, 1, pad)[:, :, :-2:2][:, :, :-2:2].shape[2]      # the encoder's frame count of the padded input
        ref = C.search(lambda tok, t, par: np.tile(bias, (2, 1)), 2, maxlen, sos, eos)
        assert ref["steps"] == maxlen - 1 and (ref["best_hyps"] == 3).all()
        want.append("%s %s" % (uttid, "".join(str(c) for c in P.ids_to_text(ref["best_hyps"].tolist(), eos, char_dict))))
    assert len(want) == 3 and all(ln.split(" ")[1].strip(char_dict[5]) == "" and len(ln.split(" ")[1]) > 8 for ln in want)
    lines = []
    mean, results = P.predict(cfg, log=lines.append, model=model)
    got = (tmp_path / "exp" / "test_attention" / "result.txt").read_text().splitlines()
    assert got == want, (got, want)
    assert ["%s %s" % (u, t) for u, t, _ in results] == want
    assert sum(ln.startswith("cer : ") for ln in lines) == 3 and lines[-1].startswith("cer_average : ")
    assert sum(ln.startswith("Hyps (") for ln in lines) == 3 and sum(ln.startswith("Labs (") for ln in lines) == 3
    # through a checkpoint file
    os.makedirs(str(tmp_path / "exp" / "model"), exist_ok=True)
    write_mindspore_ckpt(str(tmp_path / "exp" / "model" / "avg.ckpt"), to_reference_names(model.state_dict()))
    os.remove(str(tmp_path / "exp" / "test_attention" / "result.txt"))
    P.predict(cfg, log=lambda _l: None)
    assert (tmp_path / "exp" / "test_attention" / "result.txt").read_text().splitlines() == want
    # the host-stepped form is not built
    rest = {k: v for k, v in cfg.items() if k != "full_graph"}
    for fg in ({"full_graph": False}, {}):
        with pytest.raises(NotImplementedError):
            P.predict(dict(rest, **fg), log=lambda _l: None, model=model)
