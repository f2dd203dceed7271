"""CPU: the FastSpeech2 restatement against independent formulas, the checkpoint name map, the public interface, the header and the
script's front end.  Nothing here touches a device."""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fastspeech2_cases as fc  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_sinusoid_table_matches_closed_form():
    from mindaudio_amd.models.fastspeech2 import sinusoid_table

    t = sinusoid_table(65, 64)
    ref = fc.sinusoid_closed_form(65, 64)
    assert t.dtype == np.float32 and t.shape == (65, 64)
    assert np.array_equal(t, ref)
    assert np.all(t[0, 0::2] == 0.0) and np.all(t[0, 1::2] == 1.0)
    assert abs(float(t[3, 0]) - np.sin(3.0)) < 1e-7 and abs(float(t[3, 1]) - np.cos(3.0)) < 1e-7


def test_length_regulator_matches_repeat():
    ids = np.array([[5, 6, 7, 0], [9, 8, 0, 0], [4, 0, 0, 0]])
    dur = np.array([[2, 0, 3, 0], [0, 0, 0, 0], [6, 0, 0, 0]], np.float32)
    out, mel_len = fc.length_regulate(ids, dur)
    assert mel_len.tolist() == [5, 0, 6] and out.shape == (3, 6)
    assert out[0].tolist() == [5, 5, 7, 7, 7, 0] and out[1].tolist() == [0] * 6 and out[2].tolist() == [4] * 6
    for b in range(3):
        assert np.array_equal(out[b, :mel_len[b]], np.repeat(ids[b], dur[b].astype(np.int32)))


def test_duration_rounding_rule():
    # exp(log(1 + v)) - 1 = v up to float32 rounding: half-integers go to the even neighbour, negative values clip to 0
    for v, want in ((0.5, 0.0), (1.5, 2.0), (2.5, 2.0), (3.5, 4.0), (0.49, 0.0), (0.51, 1.0)):
        e = np.float32(1.0 + v)  # exactly representable
        assert np.rint(e - np.float32(1.0)) == want
    logd = np.array([-3.0, -0.1, 0.0, np.log(4.0)], np.float32)
    assert fc.round_durations(logd, 1.0).tolist() == [0.0, 0.0, 0.0, 3.0]
    assert fc.round_durations(logd, 1.5).tolist() == [0.0, 0.0, 0.0, 4.5]  # the control multiplies after the rounding
    assert fc.round_durations(np.array([-3.0], np.float32), -1.0).tolist() == [1.0]  # round(-0.95) = -1, * -1, clip


def test_bins_and_searchsorted_side():
    from mindaudio_amd.models.fastspeech2 import variance_bins

    pb, eb = fc.bins_from_stats(fc.YAML)
    p2, e2 = variance_bins((0.0, 843.436831, 0.0436493270, 494.149902), 256)
    assert np.array_equal(pb, p2) and np.array_equal(eb, e2) and pb.shape == (255,) and pb.dtype == np.float32
    assert abs(float(pb[0]) - 1e-5) < 1e-11 and abs(float(pb[-1]) - 843.436841) < 1e-3  # log with + 1e-5
    assert np.allclose(np.diff(np.log(pb.astype(np.float64))), np.log(843.436841 / 1e-5) / 254, rtol=1e-4)
    assert abs(float(eb[0]) - 0.0436493270) < 1e-8 and np.allclose(np.diff(eb.astype(np.float64)), (494.149902 - 0.0436493270) / 254, rtol=1e-4)
    # side left: a value equal to an edge gets that edge's index, i.e. #{bins < v}
    v = np.array([eb[3], np.nextafter(eb[3], np.float32(np.inf)), -1.0, 1e9], np.float32)
    idx = np.searchsorted(eb, v, "left")
    assert idx.tolist() == [3, 4, 0, 255] and idx.tolist() == [int((eb < x).sum()) for x in v]


def test_group_norm_matches_torch():
    g = torch.Generator().manual_seed(0)
    x = torch.randn((3, 7, 64), generator=g, dtype=torch.float64) * 3 + 1
    gamma, beta = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    ours = fc.group_norm(x, 8, gamma, beta)
    ref = torch.nn.functional.group_norm(x.transpose(1, 2)[..., None], 8, gamma, beta, 1e-5)[..., 0].transpose(1, 2)
    assert torch.allclose(ours, ref, rtol=0, atol=1e-12)


def test_masked_softmax_matches_torch():
    g = torch.Generator().manual_seed(1)
    s = torch.randn((2, 2, 5, 6), generator=g, dtype=torch.float64)
    mask = torch.tensor([[False, False, False, True, True, True], [False] * 6])[:, None, None, :]
    e, l = fc.masked_softmax(s, mask)
    ref = torch.softmax(s.masked_fill(mask, -float("inf")), -1)
    assert torch.allclose(e / l, ref, rtol=0, atol=1e-15) and bool((e[0, :, :, 3:] == 0).all())
    e, l = fc.masked_softmax(s, torch.ones((2, 1, 1, 6), dtype=torch.bool))
    assert bool((e == 0).all()) and bool((l == 0).all())  # the stated departure: zeros, not NaN


def test_restatement_runs_and_expands():
    texts, lens = fc.make_inputs(fc.SMALL, [1, 5, 12], seed=3)
    out = fc.infer(fc.SMALL, fc.make_state(fc.SMALL, 0), texts, lens)
    T = out["mel_predictions"].shape[1]
    assert out["mel_predictions"].shape == (3, T, 16) and out["log_duration_predictions"].shape == (3, 12)
    d = out["duration_rounded"]
    assert 2.0 <= d[2].mean() <= 4.0 and np.all(d[0, 1:] == 0) and out["mel_len"].tolist() == d.sum(1).astype(int).tolist()
    assert np.all(np.isfinite(out["mel_predictions"]))
    # padded frames take part: the adaptor's predictions there are not zero
    assert np.abs(out["pitch_predictions"][0, int(out["mel_len"][0]):]).max() > 0


def test_public_class_and_signature():
    from mindaudio_amd import models

    assert hasattr(models, "FastSpeech2")
    want = ["speakers", "texts", "src_lens", "max_src_len", "positions_encoder", "positions_decoder", "mel_lens", "max_mel_len", "p_targets",
            "e_targets", "d_targets", "p_control", "e_control", "d_control"]
    params = list(inspect.signature(models.FastSpeech2.infer).parameters)
    assert params[1:1 + len(want)] == want and params[-1] == "_overrides"
    m = models.FastSpeech2(fc.SMALL)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {k: tuple(v) for k, v in fc.param_shapes(fc.SMALL).items()}
    with pytest.raises(NotImplementedError, match="forward"):
        m.forward(None)
    with pytest.raises(NotImplementedError, match="forward_expanded"):
        m.forward_expanded(None)
    with pytest.raises(NotImplementedError, match="use_fp16"):
        models.FastSpeech2(fc.H(dict(fc.SMALL, use_fp16=True)))
    with pytest.raises(NotImplementedError, match="phoneme_level"):
        models.FastSpeech2(fc.H(dict(fc.SMALL, pitch=dict(fc.SMALL["pitch"], feature="phoneme_level"))))
    m2 = models.FastSpeech2(fc.SMALL, stats=(1.0, 100.0, 2.0, 50.0), norm="layer")
    assert abs(float(m2.variance_adaptor.energy_bins[0]) - 2.0) < 1e-6 and m2.groups == 0
    assert list(m2.state_dict()) == list(m.state_dict())  # the parameter names are the same for both norms


def test_checkpoint_names_round_trip(tmp_path):
    from mindaudio_amd import models
    from mindaudio_amd.utils import ckpt

    state = fc.make_state(fc.SMALL, 5)
    ref = ckpt.fastspeech2_to_reference_names(state)
    assert "variance_adaptor.pitch_bins_log" in ref and "variance_adaptor.energy_bins" in ref
    assert "encoder.src_word_emb.embedding_table" in ref and "variance_adaptor.pitch_embedding.embedding_table" in ref
    assert ref["encoder.layer_stack.0.pos_ffn.w_1.weight"].shape == (128, 64, 1, 9)
    assert ref["variance_adaptor.duration_predictor.conv1.0.weight"].shape == (64, 64, 1, 3)
    path = str(tmp_path / "fs2.ckpt")
    ckpt.write_mindspore_ckpt(path, ref)
    back = ckpt.convert_fastspeech2_names(ckpt.read_mindspore_ckpt(path))
    assert sorted(back) == sorted(state)
    for k, v in state.items():
        assert np.array_equal(np.asarray(back[k]), v.numpy()), k
    m = models.FastSpeech2(fc.SMALL)
    assert ckpt._is_fastspeech2(m)
    missing, unexpected = ckpt.load_mindspore_checkpoint(m, path)
    assert not missing and not unexpected
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k
    # the bare parameter names and a checkpoint without bins
    bare = {("pitch_bins_log" if k.endswith("pitch_bins_log") else k): v for k, v in ref.items() if not k.endswith("energy_bins")}
    ckpt.write_mindspore_ckpt(path, bare)
    m = models.FastSpeech2(fc.SMALL, stats=(1.0, 100.0, 2.0, 50.0))
    missing, unexpected = ckpt.load_mindspore_checkpoint(m, path)
    assert not missing and not unexpected
    assert torch.equal(m.variance_adaptor.pitch_bins, state["variance_adaptor.pitch_bins"])
    assert abs(float(m.variance_adaptor.energy_bins[0]) - 2.0) < 1e-6  # kept from `stats`


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "mindaudio_amd.h")).read()
    from mindaudio_amd import _lib

    for sym in ("ma_mha_d128_bf16", "ma_groupnorm_stats", "ma_groupnorm_apply", "ma_length_regulate_i32", "ma_variance_head_f32",
                "ma_fs2_fft_stack", "ma_fs2_workspace_bytes", "ma_fs2_layernorm_pack_f32", "ma_fs2_embed_f32", "ma_fs2_durations_f32"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert sym in _lib.PROTOTYPES
    assert "ma_fs2_plan_t" in text and "sublayers.py" in text and "variance_adapter.py" in text


def test_front_end_maps_phonemes_to_recorded_ids():
    from mindaudio_amd.fastspeech2 import generate

    table = generate.read_symbols(os.path.join(GOLDEN, "fastspeech2_symbols.txt"))
    assert len(table) == 360 and table["_"] == 0 and table[" "] == 11
    recorded = json.load(open(os.path.join(GOLDEN, "fastspeech2_ids.json")))
    assert recorded["{HH AH0 L OW1}"] == [106, 73, 117, 123]
    for phrase, ids in recorded.items():
        assert generate.phonemes_to_sequence(phrase, table) == ids
    lex = {"hello": ["HH", "AH0", "L", "OW1"], "world": ["W", "ER1", "L", "D"]}
    assert generate.text_to_phonemes("Hello, world!", lex) == "{HH AH0 L OW1 sp W ER1 L D}"
    with pytest.raises(NotImplementedError, match="g2p_en"):
        generate.text_to_phonemes("hello there", lex)


def test_kernel_refusals_launch_nothing():
    """Every argument check comes before any HIP call: the refusals are visible without a device (the pointers are never followed)."""
    import ctypes

    from mindaudio_amd import _build, _lib

    _build.build()
    lib = _lib.load()
    p = 4096  # an aligned non-null address
    INVALID, UNSUPPORTED = _lib.MA_ERR_INVALID_ARG, _lib.MA_ERR_UNSUPPORTED
    mha = lambda dk=128, ld=256, T=8, q=p: lib.ma_mha_d128_bf16(q, ld, p, ld, p, ld, p, 2, T, T, 2, dk, 0.1, p, ld, T, None)
    assert mha(dk=48) == UNSUPPORTED and mha(ld=250) == INVALID and mha(ld=260) == UNSUPPORTED and mha(T=0) == INVALID
    assert mha(q=p + 2) == INVALID and mha(q=None) == INVALID
    assert lib.ma_groupnorm_parts(1) == 1 and lib.ma_groupnorm_parts(64) == 1 and lib.ma_groupnorm_parts(65) == 2
    assert lib.ma_groupnorm_stats(p, 2, 8, 256, 7, p, None) == UNSUPPORTED      # C % G
    assert lib.ma_groupnorm_stats(p, 2, 8, 72, 8, p, None) == UNSUPPORTED       # (C / G) % 4
    assert lib.ma_groupnorm_stats(p, 2, 8, 192, 8, p, None) == UNSUPPORTED      # C / 4 no divisor of 256
    assert lib.ma_groupnorm_stats(None, 2, 8, 256, 8, p, None) == INVALID
    assert lib.ma_groupnorm_apply(p, 2, 8, 256, 192, 8, 4, p, 1e-5, p, p, None, p, p, None) == INVALID  # Cpad < C
    assert lib.ma_groupnorm_apply(p, 2, 8, 256, 256, 8, 4, p, 1e-5, p, p, None, None, None, None) == INVALID  # no output
    assert lib.ma_fs2_layernorm_pack_f32(p, 2, 8, 96, 4, p, p, 1e-5, None, p, None, None) == UNSUPPORTED
    assert lib.ma_fs2_layernorm_pack_f32(p, 2, 8, 2048, 4, p, p, 1e-5, None, p, None, None) == UNSUPPORTED
    head = lambda F=256, table=p, x=p, bins=p, x_out=p, x_pos=None, pos=None: lib.ma_variance_head_f32(
        p, 2, 8, F, p, p, 1e-7, p, p, None, 1.0, p, bins, 16, None, p, table, x, pos, 64, 4, x_out, x_pos, None, None)
    assert head(F=100) == UNSUPPORTED and head(x=None) == INVALID and head(bins=None) == INVALID and head(x_out=None) == INVALID
    assert head(x_pos=p) == INVALID  # x_pos without pos
    assert lib.ma_fs2_embed_f32(p, 2, 8, 60, 10, 4, p, p, p, p, None) == UNSUPPORTED
    assert lib.ma_fs2_durations_f32(p, 0, 1.0, p, None) == INVALID
    assert lib.ma_length_regulate_i32(p, p, 2, 4097, None, p, p, 10, None) == UNSUPPORTED
    assert lib.ma_length_regulate_i32(p, None, 2, 8, None, p, p, 10, None) == INVALID  # an expansion needs the ids
    layers = (_lib.Fs2Layer * 1)()
    plan = lambda **kw: _lib.Fs2Plan(**{**dict(n_layers=1, heads=2, d_model=256, d_inner=1024, k1=9, groups=8, halo=4, B=2, T=8, eps=1e-5,
                                               layers=layers), **kw})
    nbytes = lib.ma_fs2_workspace_bytes(ctypes.byref(plan()))
    assert nbytes >= 2 * 16 * 768 * 2 + 2 * 8 * (256 * 2 + 256 * 4 + 1024 * 2)
    assert lib.ma_fs2_workspace_bytes(ctypes.byref(plan(halo=3))) == INVALID       # a tap would read the neighbouring utterance
    assert lib.ma_fs2_workspace_bytes(ctypes.byref(plan(heads=1))) == UNSUPPORTED  # d_k 256
    assert lib.ma_fs2_workspace_bytes(ctypes.byref(plan(d_model=200))) == UNSUPPORTED
    assert lib.ma_fs2_workspace_bytes(ctypes.byref(plan(k1=4))) == INVALID
    assert lib.ma_fs2_workspace_bytes(ctypes.byref(plan(groups=0))) == nbytes      # LayerNorm needs no more
    assert lib.ma_fs2_fft_stack(ctypes.byref(plan()), p, p, p, p, nbytes - 1, None) == _lib.MA_ERR_WORKSPACE
    assert lib.ma_fs2_fft_stack(ctypes.byref(plan()), p, p, p, p, nbytes, None) == INVALID  # a layer with null weights, before any launch
