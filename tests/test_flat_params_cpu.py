"""CPU: train.flat - the one parameter store of the four trainers.  Binding needs no device, so the layout of every flat buffer, the
views, the checkpoint round trip and the shared Adam helper are checked here; the layouts against a restatement of the rule the
trainers had when each kept its own copy (cumulative ceil8 in the trainer's name order, 64-element biases for WaveGrad's
residual_dense; cumulative ceil64 in the engine) and against the totals that commit produced."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import conv_tasnet_cases as CC
import conv_tasnet_train_cases as CT
import deepspeech2_cases as DS
import wavegrad_train_cases as WT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
KINDS = ("wavegrad", "conv_tasnet", "deepspeech2")
# FlatParams.size of each trainer at its tiny case, and the engine's size and bucket spans at (256, 512, 2, 15, 4, 19, 101): what commit
# 224a0a8 (the last one with a copy of the bookkeeping per trainer) computes on the CPU for the same models
PARENT_TOTALS = {"wavegrad": 16504, "conv_tasnet": 149120, "deepspeech2": 184128}
PARENT_ENGINE_SIZE = 3983744
PARENT_ENGINE_SPANS = [(2963200, 3957248), (1969152, 2963200), (3957248, 3983744), (0, 1969152)]
MOMENTS = {"wavegrad": ("moment1", "moment2"), "conv_tasnet": ("momentum",), "deepspeech2": ("moment1", "moment2")}


def _ceil(n, m):
    return (n + m - 1) // m * m


def _trainer(kind, seed=0, bind=True, **kw):
    """(state that went into the model, trainer) at the kind's tiny case; float32 operands, which bind without a device."""
    from mindaudio_amd import _build
    from mindaudio_amd import models as M

    _build.build()
    if kind == "wavegrad":
        hps = WT.case("tiny_b2")["hps"]
        state = WT.case("tiny_b2")["state"] if seed == 0 else WT.W.make_state(hps, 50 + seed)
        model = M.WaveGrad(hps)
        model.load_state_dict(state)
        tr = M.WaveGradTrainer(model, 1e-3, operands="f32", **kw)
    elif kind == "conv_tasnet":
        cfg = dict(CT.TINY, R=CT.CASES["k64"][1])
        state = CC.make_state(cfg, 11 + cfg["R"] + seed)
        model = M.ConvTasNet(**cfg, overlap="paired")
        model.load_state_dict(state)
        tr = M.ConvTasNetTrainer(model, operands="f32", **dict(dict(momentum=0.9), **kw))
    else:
        cfg = DS.SMALL
        state = DS.make_state(cfg, 11 + seed)
        model = M.DeepSpeechModel(batch_size=cfg["B"], labels=DS.LABELS, rnn_hidden_size=cfg["H"], nb_layers=cfg["layers"],
                                  audio_conf=dict(sample_rate=cfg["sample_rate"], window_size=cfg["window_size"]))
        model.load_weights(state)
        tr = M.DeepSpeech2Trainer(model, 3e-4, 1e-5, **kw)
    if bind:
        tr._bind(CPU)
    return state, tr


def _parent_rule(kind, model):
    """[(name, numel, reserved elements)] in the flat order of the trainer's own bookkeeping, as it was."""
    params = dict(model.named_parameters())
    if kind == "wavegrad":
        wide = {id(blk.residual_dense) for blk in list(model.DBlock)[1:]}
        out = []
        for name, conv in model.named_modules():
            if isinstance(conv, nn.Conv1d):
                out.append((name + ".weight", conv.weight.numel(), conv.weight.numel()))
                out.append((name + ".bias", conv.bias.numel(), _ceil(conv.bias.numel(), 64) if id(conv) in wide else conv.bias.numel()))
        return out
    if kind == "conv_tasnet":
        return [(name, p.numel(), p.numel()) for name, p in params.items()]
    names = ["RNN.lstms.%d.%s_l0%s" % (k, leaf, suffix) for k in range(model.hidden_layers) for suffix in ("", "_reverse")
             for leaf in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + ["fc.module.weight"]
    return [(name, params[name].numel(), params[name].numel()) for name in names]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. layout parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_model_trainer_layout_is_the_parents(kind):
    _, tr = _trainer(kind)
    fp, off, want = tr.params, 0, {}
    for name, n, reserved in _parent_rule(kind, tr.model):
        want[name] = (off, n)
        off += _ceil(reserved, 8)
    assert list(fp.index) == list(want)
    assert {name: (o, n) for name, (o, _, n) in fp.index.items()} == want
    assert fp.size == off == PARENT_TOTALS[kind]
    assert fp.pad == 8 and fp.moments == MOMENTS[kind]
    for buf in (fp.master, fp.grad) + tuple(getattr(fp, m) for m in fp.moments):
        assert buf.dtype == torch.float32 and buf.numel() == fp.size and buf.is_contiguous()
    assert fp.bf16 is fp.master  # float32 operands: no mirror


def test_wavegrad_has_the_wide_biases():
    _, tr = _trainer("wavegrad")
    wide = [(name, n, r) for name, n, r in _parent_rule("wavegrad", tr.model) if r != n]
    assert wide and all(name.endswith("residual_dense.bias") and r == 64 and n < 64 for name, n, r in wide)


def test_engine_layout_is_the_parents():
    from mindaudio_amd.train import engine, flat

    assert engine.FlatParams is flat.FlatParams and engine.DynamicLossScale is flat.DynamicLossScale
    entries = engine.conformer_ctc_entries(256, 512, 2, 15, 4, 19, 101)
    fp = engine.FlatParams(entries, "cpu")
    off, want = 0, {}
    for name, shape in entries:
        n = int(np.prod(shape))
        want[name] = (off, tuple(shape), n)
        off += _ceil(n, 64)
    assert fp.index == want and list(fp.index) == [name for name, _ in entries]
    assert fp.size == off == PARENT_ENGINE_SIZE
    assert [tuple(s) for s in engine.bucket_spans(fp, 2)] == PARENT_ENGINE_SPANS
    assert fp.moments == ("exp_avg", "exp_avg_sq") and fp.exp_avg.numel() == fp.exp_avg_sq.numel() == fp.size
    assert fp.bf16.dtype == torch.bfloat16 and fp.bf16.numel() == fp.size
    assert engine.FlatParams(entries[:3], "cpu", mirror_bf16=False).bf16.dtype == torch.float32
    # one allocation: the flag sits behind the gradient, so that one fill zeroes both
    assert fp.flag.dtype == torch.int32 and fp.flag.data_ptr() == fp.grad.data_ptr() + 4 * fp.size
    assert fp.flag.data_ptr() < fp._grad_alloc.data_ptr() + 4 * fp._grad_alloc.numel()
    assert fp.p("conv1_w") is fp.p("conv1_w") and fp.g("ctc_b") is fp.g("ctc_b") and fp.w("pos_w") is fp.w("pos_w")  # cached


def test_store_options_on_a_hand_made_layout():
    from mindaudio_amd.train.flat import FlatParams, stored_last_first, stored_taps_inner

    fp = FlatParams([("a", (4, 1, 3), stored_last_first), ("b", (2, 5, 3), stored_taps_inner), ("c", (5,), None, 64), ("d", (9,))], "cpu",
                    mirror_bf16=True, pad=8, moments=("m",))
    assert fp.index == {"a": (0, (4, 1, 3), 12), "b": (16, (2, 5, 3), 30), "c": (48, (5,), 5), "d": (112, (9,), 9)} and fp.size == 128
    assert fp.span(["b", "c"]) == (16, 112) and fp.span(["d"]) == (112, 128)
    assert fp.ptr("b") == fp.master.data_ptr() + 16 * 4 and fp.ptr("d", fp.m) == fp.m.data_ptr() + 112 * 4
    assert fp.ptr("b", fp.bf16) == fp.bf16.data_ptr() + 16 * 2
    fp.master.copy_(torch.arange(128.0))
    a, b = torch.arange(12.0).view(3, 4), 16 + torch.arange(30.0).view(2, 3, 5)
    assert tuple(fp.p("a").shape) == (4, 1, 3) and torch.equal(fp.p("a"), a.t().unsqueeze(1))           # stored (last, first)
    assert tuple(fp.p("b").shape) == (2, 5, 3) and torch.equal(fp.p("b"), b.permute(0, 2, 1))           # stored (N, taps, C)
    assert torch.equal(fp.p("c"), 48 + torch.arange(5.0)) and tuple(fp.w("b").shape) == (2, 5, 3)
    assert not hasattr(fp, "exp_avg")


# ---- 2. views ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_views_alias_the_master_and_padding_stays_zero(kind):
    state, tr = _trainer(kind)
    fp = tr.params
    assert fp.size % fp.pad == 0 and all(off % fp.pad == 0 for off, _, _ in fp.index.values())
    used = torch.zeros(fp.size, dtype=torch.bool)
    for off, _, n in fp.index.values():
        assert not used[off:off + n].any()  # no two entries overlap
        used[off:off + n] = True
    assert not fp.master[~used].any()  # padding and reserved tails: zero after the bind
    params = dict(tr.model.named_parameters())
    for name, (off, shape, n) in fp.index.items():
        assert tuple(params[name].shape) == shape and torch.equal(params[name].detach(), torch.as_tensor(state[name]).float())
        assert torch.equal(fp.p(name), params[name].detach()) and tuple(tr.gradients()[name].shape) == shape
    for i, name in enumerate(fp.index):  # writing through the model's parameter changes the flat buffer, and only that entry
        params[name].data.fill_(float(i + 2))
    for i, (off, _, n) in enumerate(fp.index.values()):
        assert bool((fp.master[off:off + n] == float(i + 2)).all())
    assert not fp.master[~used].any()


def test_both_layouts_against_the_state_dict_tensors():
    state, tr = _trainer("wavegrad")
    fp, sd = tr.params, tr.state_dict()
    convs = [n for n in fp.index if n.endswith(".weight") and n != "DBlock.0.weight"]
    assert len(convs) > 10 and "last_conv.weight" in convs
    for name in convs:  # stored (N, taps, C), seen (N, C, taps)
        off, (N, C, taps), n = fp.index[name]
        assert torch.equal(fp.master[off:off + n].view(N, taps, C), state[name].permute(0, 2, 1))
        assert torch.equal(sd[name], state[name]) and sd[name].is_contiguous()
    off, (C0, one, taps), n = fp.index["DBlock.0.weight"]  # stored (taps, C0), seen (C0, 1, taps)
    assert one == 1 and torch.equal(fp.master[off:off + n].view(taps, C0), state["DBlock.0.weight"][:, 0, :].t())
    assert torch.equal(sd["DBlock.0.weight"], state["DBlock.0.weight"])
    state, tr = _trainer("conv_tasnet")
    fp, sd = tr.params, tr.state_dict()
    tap_major = [n for n in fp.index if n.endswith(("depthwise_conv.weight", "conv1d_U.weight"))]
    assert len(tap_major) == 9
    for name in tap_major:
        off, (first, one, last), n = fp.index[name]
        assert one == 1 and torch.equal(fp.master[off:off + n].view(last, first), state[name][:, 0, :].t())
        assert torch.equal(sd[name], state[name]) and sd[name].is_contiguous()


# ---- 3. state ---------------------------------------------------------------------------------------------------------------------------
def _fill_moments(tr, seed):
    g = torch.Generator().manual_seed(seed)
    for m in tr.params.moments:
        for name in tr.params.index:
            v = tr.params._view(getattr(tr.params, m), name)
            v.copy_(torch.randn(v.shape, generator=g))


@pytest.mark.parametrize("bound", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_state_round_trip_is_bit_exact(kind, bound):
    state, src = _trainer(kind)
    _fill_moments(src, 5)
    src.steps = 3
    if kind == "wavegrad":
        src.scaler.scale = 512.0
    sd = src.state_dict()
    trained = list(src.params.index)
    extra = {"steps"} | ({"loss_scale"} if kind == "wavegrad" else set())
    assert set(sd) == set(src.model.state_dict()) | {"%s.%s" % (m, n) for m in MOMENTS[kind] for n in trained} | extra
    assert all(v.is_contiguous() for v in sd.values())
    _, dst = _trainer(kind, seed=1, bind=bound)
    dst.load_state_dict(sd)
    if not bound:
        assert dst.params is None  # a load binds nothing
        dst._bind(CPU)
    assert dst.steps == 3 and (kind != "wavegrad" or dst.scaler.scale == 512.0)
    assert torch.equal(_bits(dst.params.master), _bits(src.params.master))
    for m in MOMENTS[kind]:
        for name in trained:
            got, want = dst.params._view(getattr(dst.params, m), name), src.params._view(getattr(src.params, m), name)
            assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(sd["%s.%s" % (m, name)]), _bits(want)), (m, name)
    again = dst.state_dict()
    assert list(again) == list(sd) and all(torch.equal(again[k], sd[k]) for k in sd)
    assert not hasattr(src, "_pending_momentum") and not hasattr(dst, "_pending_momentum") and dst._pending is None


def test_an_unbound_trainer_saves_no_moments_and_absent_keys_are_ignored():
    _, tr = _trainer("deepspeech2", bind=False)
    sd = tr.state_dict()
    assert set(sd) == set(tr.model.state_dict()) | {"steps"}
    _, bound = _trainer("deepspeech2", seed=1)
    _fill_moments(bound, 7)
    keep = [bound.params.moment1.clone(), bound.params.moment2.clone()]
    bound.load_state_dict(sd)  # no moment keys: the moments stay
    assert torch.equal(bound.params.moment1, keep[0]) and torch.equal(bound.params.moment2, keep[1])
    half = dict(bound.state_dict())
    del half["moment2.fc.module.weight"]
    half["moment1.fc.module.weight"] = half["moment1.fc.module.weight"].double().numpy()  # another dtype, not a tensor
    _, other = _trainer("deepspeech2", seed=2)
    other.load_state_dict(half)
    assert torch.equal(other.params._view(other.params.moment1, "fc.module.weight"), bound.params._view(bound.params.moment1, "fc.module.weight"))
    assert not other.params._view(other.params.moment2, "fc.module.weight").any()


def test_conv_tasnet_without_momentum_has_no_momentum_keys():
    _, with_m = _trainer("conv_tasnet")
    _fill_moments(with_m, 3)
    _, tr = _trainer("conv_tasnet", momentum=0.0)
    assert tr.params.moments == () and not hasattr(tr.params, "momentum")
    sd = tr.state_dict()
    assert set(sd) == set(tr.model.state_dict()) | {"steps"}
    tr.load_state_dict(with_m.state_dict())  # momentum entries of another run: nowhere to go
    assert set(tr.state_dict()) == set(sd) and not hasattr(tr, "_pending_momentum")


# ---- 4. the shared Adam helper ----------------------------------------------------------------------------------------------------------
def test_adam_lr_t_keeps_its_bits():
    from mindaudio_amd.train.flat import ADAM_BETA1, ADAM_BETA2, adam_lr_t

    assert ADAM_BETA1 == float(np.float32(0.9)) and ADAM_BETA2 == float(np.float32(0.999)) and ADAM_BETA2 != 0.999
    for b1, b2 in ((0.9, 0.999), (ADAM_BETA1, ADAM_BETA2)):
        for lr in (1e-3, 3e-4):
            for t in range(1, 6):
                assert adam_lr_t(lr, t, b1, b2) == lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


# ---- 5. the import edge -----------------------------------------------------------------------------------------------------------------
def test_the_wavegrad_trainer_does_not_import_the_conformer_engine():
    code = ("import sys; import mindaudio_amd.models.wavegrad_train as w; from mindaudio_amd.train import flat; "
            "assert w.DynamicLossScale is flat.DynamicLossScale; "
            "print('engine' if 'mindaudio_amd.train.engine' in sys.modules else 'clean')")
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable] + flags + ["-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode(errors="replace")
    assert out.stdout.decode().strip() == "clean"
