"""CPU proof of tests/attn_decode_cases.py and of the host side of the `attention` decode mode: the float64 beam step reproduces
the reference's recorded steps exactly, the KV-cached decoder restatement is the reference's full-prefix step, every comparator
rejects its planted defect, the end-to-end cases clear their guard, the three entry points are declared, exported and bound, and
the mode's refusals are raised without a device."""
import os
import re

import numpy as np
import pytest

import attn_decode_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRY_POINTS = ("ma_decoder_self_attn_step_bf16", "ma_attn_beam_step_f32", "ma_attn_beam_best_f32")


@pytest.fixture(scope="module")
def gold():
    return C.goldens()


def test_fixture_holds_the_cases_the_search_can_go_wrong_on(gold):
    names = C.golden_names(gold)
    beams = {int(gold[n + "_beam"]) for n in names}
    assert beams == {1, 4, 10, 16}
    assert any(int(gold[n + "_V"]) == int(gold[n + "_beam"]) for n in names)
    assert {int(gold[n + "_maxlen"]) for n in names} >= {2, 3}
    n = "length_limit"
    assert int(gold[n + "_steps"]) == int(gold[n + "_maxlen"]) - 1 and not gold[n + "_end_out"].any()
    assert int(gold["all_finish_first_step_steps"]) == 1 and int(gold["all_finish_step1_steps"]) == 2
    # beams that finish at different steps, -inf rows at the first step, the -10000 branches inside a beam
    assert any(((gold[n + "_end_in"].sum(1) > 0) & (gold[n + "_end_in"].sum(1) < int(gold[n + "_beam"]))).sum() >= 2 for n in names)
    assert all(np.isneginf(gold[n + "_scores_in"][0][1:]).all() for n in names)
    assert any((gold[n + "_scores_out"] < -5000).any() for n in names)
    for n in names:  # log_softmax is the identity on the recorded logits: any implementation gives the same log-probabilities
        lg = gold[n + "_logits"]
        assert (lg.max(-1) == 0).all() and (np.sort(lg, -1)[..., -2] <= -30).all() if lg.shape[-1] > 1 else True
        m = lg.max(-1, keepdims=True)
        lp32 = (lg - m) - np.log(np.exp(lg - m).sum(-1, keepdims=True, dtype=np.float32))
        assert lp32.dtype == np.float32 and np.array_equal(lp32, lg)


def test_beam_step_reproduces_every_recorded_step(gold):
    for name in C.golden_names(gold):
        p = name + "_"
        eos, steps = int(gold[p + "eos"]), int(gold[p + "steps"])
        for dtype in (np.float64, np.float32):
            for s in range(steps):
                ins, want, n, maxlen = C.golden_step(gold, name, s)
                # the top-k lists are the stable top-k of the recorded logits' float32 log_softmax
                lp, ix = C.topk_rows(C.log_softmax(gold[p + "logits"][s]), n)
                assert np.array_equal(lp.astype(np.float32), ins["tk_logp"]) and np.array_equal(ix, ins["tk_index"])
                got = C.beam_step(ins["tk_logp"], ins["tk_index"], ins["scores_in"], ins["end_in"], ins["tokens_in"], s, 0, eos,
                                  maxlen - 1, dtype)
                C.check_beam(got[:7], want)


def test_search_reproduces_every_final_result(gold):
    for name in C.golden_names(gold):
        p = name + "_"
        logits = gold[p + "logits"]
        res = C.search(lambda tok, t, par: logits[t], int(gold[p + "beam"]), int(gold[p + "maxlen"]), int(gold[p + "sos"]),
                       int(gold[p + "eos"]), dtype=np.float32)
        assert res["steps"] == int(gold[p + "steps"])
        assert np.array_equal(res["best_hyps"], gold[p + "best_hyps"]), name
        assert np.float32(res["best_score"]) == gold[p + "best_score"], name


def test_frozen_utterance_is_copied_through(gold):
    ins, want, n, maxlen = C.golden_step(gold, "beam4", 3)
    got = C.beam_step(ins["tk_logp"], ins["tk_index"], ins["scores_in"], ins["end_in"], ins["tokens_in"], 3, 1, int(gold["beam4_eos"]),
                      maxlen - 1)
    C.check_beam(got[:7], (ins["scores_in"], ins["end_in"], ins["tokens_in"], np.arange(n), np.full(n, int(gold["beam4_eos"])), 3, 1))


def _walk(dec, memory, mask, rows, group, maxlen, vocab, seed, defect=None):
    """Random tokens and random beam reorders: the cached step's logits and the reference-form logits of every step."""
    rng = np.random.RandomState(seed)
    cache = dec.init_cache(memory, mask, group, maxlen)
    ids = np.zeros((rows, maxlen), np.int64)
    ids[:, 0] = vocab - 1
    mem_r = np.repeat(memory, group, 0)
    mask_r = None if mask is None else np.repeat(mask, group, 0)
    out, parent = [], None
    for t in range(maxlen - 1):
        got = dec.step(cache, ids[:, t], t, parent, defect=defect)
        want = dec.reference_step(mem_r, mask_r, ids, t + 1)
        out.append((got, want))
        # the next step's rows: a reorder inside every utterance (children may share a parent), then a new token each
        parent = np.concatenate([u * group + rng.randint(0, group, size=group) for u in range(rows // group)])
        ids = ids[parent]
        ids[:, t + 1] = rng.randint(0, vocab, size=rows)
    return out


def test_cached_step_is_the_reference_full_prefix_step():
    vocab, rows, group, frames = 21, 6, 3, 11
    rng = np.random.RandomState(5)
    memory = rng.randn(rows // group, frames, C.D)
    mask = np.ones((rows // group, frames), bool)
    mask[1, frames - 3:] = False
    dec = C.Decoder(C.random_weights(11, vocab))
    for got, want in _walk(dec, memory, mask, rows, group, frames, vocab, 3):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # and the comparator of the two forms rejects the planted cache defects
    for defect in ("copy_self", "no_append"):
        pairs = _walk(dec, memory, mask, rows, group, frames, vocab, 3, defect=defect)
        assert max(np.abs(g - w).max() for g, w in pairs) > 1e-6, defect


def test_cache_comparators_reject_planted_defects():
    for R, lmax in ((4, 9), (10, 70)):
        oh = C.OneHot(R, lmax)
        k_in, v_in = oh.k_in.astype(np.float64), oh.v_in.astype(np.float64)
        for t in (1, lmax - 1):
            # (shift 1: every row's parent is another row; shift t: row 0's target is the appended position)
            for defect, shift in ((None, 1), (None, t), ("copy_self", 1), ("no_append", t)):
                qkv, parent, want_ctx, want_k, want_v = oh.case(t, shift)
                got = C.self_attn_step(qkv.astype(np.float64), k_in, v_in, parent, t, C.HEADS, 1.0 / 64, defect=defect)
                if defect is None:  # the restatement passes its own construction, exactly
                    C.check_cache(got[1], got[2], want_k, want_v, t)
                    C.check_ctx_exact(got[0], want_ctx)
                    continue
                with pytest.raises(AssertionError):
                    C.check_cache(got[1], got[2], want_k, want_v, t)
                with pytest.raises(AssertionError):
                    C.check_ctx_exact(got[0], want_ctx)
    # the random case's bound rejects a context taken from the wrong parent
    rng = np.random.RandomState(0)
    R, lmax, t, d = 10, 70, 40, 256
    qkv, k_in, v_in = (C.bf16(rng.randn(*s)) for s in ((R, 3 * d), (R, lmax, d), (R, lmax, d)))
    parent = rng.permutation(R).astype(np.int32)
    good = C.self_attn_step(qkv, k_in, v_in, parent, t, 4, 1.0 / 64)
    bad = C.self_attn_step(qkv, k_in, v_in, parent, t, 4, 1.0 / 64, defect="copy_self")
    C.check_ctx_close(good[0], good[0], good[2][:, :t + 1])
    with pytest.raises(AssertionError):
        C.check_ctx_close(bad[0], good[0], good[2][:, :t + 1])


def test_beam_comparator_rejects_planted_defects(gold):
    def run(name, s, defect, done=0, length=None):
        ins, want, n, maxlen = C.golden_step(gold, name, s)
        got = C.beam_step(ins["tk_logp"], ins["tk_index"], ins["scores_in"], ins["end_in"], ins["tokens_in"], s if length is None else length,
                          done, int(gold[name + "_eos"]), maxlen - 1, np.float32, defect)
        return got[:7], want

    # a finished row's first branch not zeroed: the goldens' best log-probability is 0 everywhere, so a step written by hand - a
    # finished row whose top-k list starts at -0.5 must keep its score
    tk_logp = np.array([[-0.5, -1.0], [-0.25, -2.0]], np.float32)
    tk_index = np.array([[3, 1], [2, 0]], np.int32)
    args = (tk_logp, tk_index, np.array([-1.0, -1.125], np.float32), np.array([1, 0]), np.array([[4, 4, 0], [4, 1, 0]], np.int32), 1, 0,
            4, 2, np.float32)
    want = C.beam_step(*args)[:7]
    C.check_beam(want, (np.array([-1.0, -1.375], np.float32), [1, 0], [[4, 4, 4], [4, 1, 2]], [0, 1], [4, 2], 2, 1))
    with pytest.raises(AssertionError):
        C.check_beam(C.beam_step(*args, "no_zero")[:7], want)
    # -inf instead of -10000: the case whose -10000 branches enter the beam ahead of the -inf candidates
    rejected = 0
    for s in range(int(gold["neg10000_in_beam_steps"])):
        got, want = run("neg10000_in_beam", s, "neg_inf")
        try:
            C.check_beam(got, want)
        except AssertionError:
            rejected += 1
    assert rejected >= 1
    # ties broken high index first
    rejected = 0
    for s in range(int(gold["ties_steps"])):
        got, want = run("ties", s, "ties_high")
        try:
            C.check_beam(got, want)
        except AssertionError:
            rejected += 1
    assert rejected >= 1
    # a frozen utterance whose length advances
    ins, _, n, maxlen = C.golden_step(gold, "beam4", 2)
    frozen = (ins["scores_in"], ins["end_in"], ins["tokens_in"], np.arange(n), np.full(n, int(gold["beam4_eos"])), 2, 1)
    got = C.beam_step(ins["tk_logp"], ins["tk_index"], ins["scores_in"], ins["end_in"], ins["tokens_in"], 2, 1, int(gold["beam4_eos"]),
                      maxlen - 1, np.float32, "frozen_length")
    with pytest.raises(AssertionError):
        C.check_beam(got[:7], frozen)


@pytest.fixture(scope="module")
def e2e():
    return [C.e2e_reference(*case)[3] for case in C.E2E]


def test_end_to_end_cases_clear_the_guard(e2e):
    kept = [r for r in e2e if r["min_gap"] > C.GUARD]
    assert len(kept) >= 6, [r["min_gap"] for r in e2e]
    assert {case[2] for case, r in zip(C.E2E, e2e) if r["min_gap"] > C.GUARD} >= {1, 2}     # beam sizes among the kept
    assert any(r["length"] < case[3] - 1 for case, r in zip(C.E2E, e2e) if r["min_gap"] > C.GUARD)  # a search that eos ends
    assert any(r["length"] == case[3] - 1 for case, r in zip(C.E2E, e2e) if r["min_gap"] > C.GUARD)  # one the length limit ends


def test_guard_is_four_times_the_rounding_noise(e2e):
    noise = max(r["noise"] for r in e2e)
    assert abs(noise - C.GUARD_MEASURED) <= 2e-3, noise
    assert 4 * C.GUARD_MEASURED <= C.GUARD <= 4.05 * C.GUARD_MEASURED


def test_bf16_rounding_is_round_to_nearest_even():
    import torch

    x = np.concatenate([np.random.RandomState(0).randn(4096) * 10.0 ** np.random.RandomState(1).randint(-6, 6, 4096),
                        [1.00390625, 1.01171875, -1.00390625, 0.0, 65280.0]])
    want = torch.from_numpy(x).float().bfloat16().double().numpy()
    assert np.array_equal(C.bf16(x), want)


def test_entry_points_declared_exported_and_bound():
    from mindaudio_amd import _build, _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mindaudio_amd.h")).read(), flags=re.S)
    _build.build()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.ABI_VERSION == 4  # new entry points alone do not bump the version


def test_mode_refusals_need_no_device():
    import torch

    from mindaudio_amd.conformer import asr_model as A
    from mindaudio_amd.conformer import predict as P

    cfg = {"decode_mode": "attention", "model_conf": {"ctc_weight": 0.3}, "dict": "/nonexistent", "test_data": "/nonexistent"}
    for fg in ({}, {"full_graph": False}):
        with pytest.raises(NotImplementedError, match="full_graph: true"):
            P.predict(dict(cfg, **fg), log=lambda _l: None)
    with pytest.raises(NotImplementedError, match="pure CTC"):
        P.predict(dict(cfg, full_graph=True, model_conf={"ctc_weight": 1.0}), log=lambda _l: None)

    class _PureCtc:
        decoder = None

    with pytest.raises(NotImplementedError):
        P.predict(dict(cfg, full_graph=True), log=lambda _l: None, model=_PureCtc())
    with pytest.raises(NotImplementedError):
        A.Attention(_PureCtc(), 4, 7)
    with pytest.raises(NotImplementedError):
        A.Attention(torch.nn.Linear(1, 1), 4, 7, pretrained_model=True)
    with pytest.raises(NotImplementedError, match="full_graph"):
        A.recognize(None, torch.zeros(1, 8, 2), torch.ones(1, 1, 8), np.array([7]), None, np.zeros(4), np.zeros(4), 4, 7,
                    full_graph=False)
    # --full_graph is a flag of the script
    seen = {}
    orig = P.predict
    try:
        P.predict = lambda config: seen.update(config)
        from mindaudio_amd.conformer import train as T

        load = T.load_config
        T.load_config = lambda path, over: dict(over)
        try:
            P.main(["--config_path", "x.yaml", "--decode_mode", "attention", "--full_graph"])
        finally:
            T.load_config = load
    finally:
        P.predict = orig
    assert seen == {"decode_mode": "attention", "full_graph": True}
