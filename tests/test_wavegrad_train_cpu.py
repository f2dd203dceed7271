"""CPU: the reference side of WaveGrad training (wavegrad_train_cases.py) and everything of the product that needs no device - the
refusals, the symbol table, the learning-rate schedule, the dataset functions against the reference's own results
(tests/golden/wavegrad_train_goldens.npz, written by gen_wavegrad_train_goldens.py), the checkpoint files of the script."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import wavegrad_cases as W  # noqa: E402
import wavegrad_train_cases as T  # noqa: E402


# ---- the restated network ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16_operands,conv", [(False, T.plain_conv), (True, T.rounded_conv), (True, T.bf16_conv)])
def test_network_is_wavegrad_cases_network_bit_for_bit(bf16_operands, conv):
    hps, shape = W.SMALL, W.SMALL_SHAPE
    state = W.make_state(hps, 3)
    audio, spec = W.inputs(hps, shape, 5)
    level = torch.tensor([0.3, 0.8])
    want = W.network(state, hps, audio, level, spec, bf16_operands=bf16_operands)
    got = T.network({k: v.double() for k, v in state.items()}, hps, audio.double(), level, spec.double(), conv)
    assert torch.equal(got, want)


def test_tiny_geometry_is_accepted_by_the_model_and_has_padded_channels():
    from mindaudio_amd.models import WaveGrad

    model = WaveGrad(T.TINY)
    assert set(W.param_shapes(T.TINY)) == set(model.state_dict())
    assert min(model.enc_dims) == 8 and all(c % 8 == 0 and c % 64 for c in model.enc_dims)
    assert sorted({T.CASES[n][1][0] for n in T.F32_CASES if n.startswith("tiny")}) == [2, 3]
    assert T.CASES["tiny_1f"][1][1] == 1


@pytest.mark.parametrize("name", T.F32_CASES)
def test_shipped_seeds_satisfy_the_guard(name):
    """No LeakyReLU input and no pred - noise within 8 x the float32 form's own error of zero, nothing excluded."""
    c = T.case(name)
    assert T.flip_margin(c["state"], c["hps"], c["batch"]) >= 1.0
    assert T.search_seed(name, tries=1) == T.SEEDS[name]  # the shipped seed is the first of its series


def test_form_c_rounds_the_gradient_where_the_device_does():
    """The custom Function rounds dY and the saved operands; the plain .to(bfloat16) chain would send an unrounded dY to dW."""
    g = torch.Generator().manual_seed(1)
    x, w, b = (torch.randn(s, generator=g, dtype=torch.float64, requires_grad=True) for s in ((2, 8, 20), (16, 8, 3), (16,)))
    dy = torch.randn((2, 16, 20), generator=g, dtype=torch.float64)
    T.bf16_conv(x, w, b, 1, 2, 2).backward(dy)
    dyr, xr, wr = T.bf16_round(dy), T.bf16_round(x.detach()), T.bf16_round(w.detach())
    assert torch.equal(w.grad, torch.nn.grad.conv1d_weight(xr, w.shape, dyr, padding=2, dilation=2))
    assert torch.equal(x.grad, torch.nn.grad.conv1d_input(x.shape, wr, dyr, padding=2, dilation=2))
    assert torch.equal(b.grad, dyr.sum(dim=(0, 2)))


# ---- the comparators reject planted defects ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", T.DEFECTS)
@pytest.mark.parametrize("name", ["tiny_b2", "small"])
def test_comparators_reject(name, defect):
    c = T.case(name)
    _, ga, _ = T.reference(name, "a")
    _, gb, _ = T.reference(name, "b")
    _, gc, _ = T.reference(name, "c")
    assert not T.check_f32(gb, ga, gb) and not T.check_bf16(gc, ga, gc)[0]  # the references pass their own checks
    _, bad64, _ = T.grads(c["state"], c["hps"], c["batch"], "a", defect=defect)
    assert T.check_f32(bad64, ga, gb), "float32 comparator accepted %s" % defect
    failures, _, cos = T.check_bf16(bad64, ga, gc)
    assert failures or cos < T.COS_MIN, "bf16 comparator accepted %s" % defect


def test_sign_of_zero_is_seen():
    """One element with pred == noise: a backward with sign(0) = 1 differs in d loss / d pred there, and only there."""
    c = T.case("tiny_b2")
    audio, level, noise, spec = c["batch"]
    _, _, aa = T.grads(c["state"], c["hps"], c["batch"], "a")
    noise2 = noise.double().clone()
    noise2[1, 7] = aa["value"][1, 7]
    batch = (audio, level, noise2, spec)
    _, g0, a0 = T.grads(c["state"], c["hps"], batch, "a")
    _, g1, a1 = T.grads(c["state"], c["hps"], batch, "a", defect="sign0")
    assert float(a0["pred"][1, 7]) == 0.0 and float(a1["pred"][1, 7]) != 0.0
    d = a0["pred"] != a1["pred"]
    assert int(d.sum()) == 1  # the comparator that sees it is the exact one on the pred gradient (test_l1_last_bwd, test_chain_f32)
    assert not torch.equal(a0["pred"], a1["pred"]) and any(not torch.equal(g0[k], g1[k]) for k in g0)


def test_clipping_before_unscaling_is_seen():
    """With a loss scale of 4096 the scaled norm is far above the clip while the unscaled one is below it: clipping first shrinks the
    step by the ratio."""
    g = torch.Generator().manual_seed(2)
    p0 = {"w": torch.randn(100, generator=g, dtype=torch.float64)}
    grads = {"w": 4096.0 * 0.01 * torch.randn(100, generator=g, dtype=torch.float64)}
    out = {}
    for defect in (None, "clip"):
        p, m1, m2 = {"w": p0["w"].clone()}, {"w": torch.zeros(100, dtype=torch.float64)}, {"w": torch.zeros(100, dtype=torch.float64)}
        for t in (1, 2):
            norm = T.clip_adam_step(p, grads, m1, m2, t, 1e-3, 4096.0, 1.0, defect)
        out[defect] = (p["w"], m1["w"], norm)
    assert out[None][2] < 1.0 < out["clip"][2]
    assert W.relrms(out["clip"][1], out[None][1]) > 0.5  # the moments are those of a gradient thousands of times smaller
    assert float((out[None][0] - p0["w"]).abs().max()) > 0


def test_clip_factor_and_adam_closed_form():
    """One element, by hand: norm 5 -> factor 0.2; first step of Adam moves by lr_t m / (sqrt v + eps) with m = (1 - b1) g, v = (1 - b2) g^2."""
    p, m1, m2 = {"w": torch.tensor([1.0], dtype=torch.float64)}, {"w": torch.zeros(1, dtype=torch.float64)}, {"w": torch.zeros(1, dtype=torch.float64)}
    norm = T.clip_adam_step(p, {"w": torch.tensor([5.0 * 8], dtype=torch.float64)}, m1, m2, 1, 0.1, 8.0, 1.0)
    assert norm == 5.0
    g = 1.0
    m, v = T.ONE_MINUS_BETA1 * g, T.ONE_MINUS_BETA2 * g * g
    lr_t = 0.1 * math.sqrt(1 - T.BETA2) / (1 - T.BETA1)
    assert abs(float(p["w"]) - (1.0 - lr_t * m / (math.sqrt(v) + T.ADAM_EPS))) < 1e-15


# ---- schedule, dataset ---------------------------------------------------------------------------------------------------------------------
def test_learning_rate_schedule():
    from mindaudio_amd.wavegrad import train as script

    got = script.exponential_decay_lr(2e-4, 0.96, 5000, 2, 1000, is_stair=True)
    want = T.exponential_decay_lr(2e-4, 0.96, 5000, 2, 1000, is_stair=True)
    assert got == want and len(got) == 5000
    assert got[0] == got[1999] == 2e-4 and got[2000] == 2e-4 * 0.96 and got[4000] == 2e-4 * 0.96 ** 2
    assert all(script.learning_rate(i, 2e-4, 2) == want[i] for i in range(0, 5000, 7))
    smooth = script.exponential_decay_lr(1.0, 0.5, 6, 2, 2, is_stair=False)
    assert smooth == [1.0, 1.0, 0.5 ** 0.5, 0.5 ** 0.5, 0.5, 0.5]
    with pytest.raises(ValueError):
        script.exponential_decay_lr(1.0, 0.5, 0, 2, 2)


def _golden():
    return np.load(os.path.join(HERE, "golden", "wavegrad_train_goldens.npz"))


def test_diffuse_and_batch_collate_are_the_references():
    """The reference's own functions under np.random.seed: the same draws in the same order, the same float32 results, bit for bit."""
    from types import SimpleNamespace

    from mindaudio_amd.wavegrad import dataset as D

    G = _golden()
    hps = SimpleNamespace(noise_schedule_start=float(G["start"]), noise_schedule_end=float(G["end"]), noise_schedule_S=int(G["S"]),
                          hop_samples=int(G["hop"]), crop_mel_frames=int(G["crop"]))
    level = D.noise_levels(hps)
    assert level.dtype == np.float32 and np.array_equal(level, G["noise_level"])
    np.random.seed(int(G["seed_diffuse"]))
    noisy, scale, noise = D.diffuse(G["x"], hps.noise_schedule_S, level)
    for got, key in ((noisy, "d_noisy"), (scale, "d_scale"), (noise, "d_noise")):
        assert np.asarray(got).dtype == G[key].dtype and np.array_equal(got, G[key]), key
    np.random.seed(int(G["seed_batch"]))
    out = D.batch_collate([G["audio_%d" % i] for i in range(3)], [G["spec_%d" % i] for i in range(3)], hps, level)
    for got, key in zip(out, ("b_noisy", "b_scale", "b_noise", "b_spec")):
        assert got.dtype == G[key].dtype and got.shape == G[key].shape and np.array_equal(got, G[key]), key
    after = np.random.rand()
    np.random.seed(int(G["seed_batch"]))
    D.batch_collate([G["audio_%d" % i] for i in range(3)], [G["spec_%d" % i] for i in range(3)], hps, level)
    assert np.random.rand() == after  # and nothing else was drawn


def test_manifest_split_and_pairs(tmp_path):
    from types import SimpleNamespace

    from mindaudio_amd.wavegrad import dataset as D

    names = []
    for i in range(200):
        wav = str(tmp_path / ("u%03d.wav" % i))
        names.append(wav)
    (tmp_path / "m.csv").write_text("".join("%s\t%s\n" % (n, n.replace(".wav", ".txt")) for n in names))
    train, held = D.read_manifest(str(tmp_path / "m.csv"), True), D.read_manifest(str(tmp_path / "m.csv"), False)
    assert len(train) == 198 and len(held) == 2 and sorted(train + held) == sorted(names) and train[:5] != sorted(names)[:5]
    order = list(names)
    np.random.seed(0)
    np.random.shuffle(order)
    assert train == order[:198]
    np.save(names[0].replace(".wav", D.WAV_POSTFIX), np.arange(5, dtype=np.float32))
    np.save(names[0].replace(".wav", D.FEATURE_POSTFIX), np.ones((8, 3), np.float32))
    x, c = D.read_pair(names[0])
    assert x.shape == (5,) and c.shape == (8, 3)
    hps = SimpleNamespace(manifest_path=str(tmp_path / "m.csv"), noise_schedule_start=1e-4, noise_schedule_end=0.05, noise_schedule_S=60)
    assert len(D.WaveGradDataset(hps, 32)) == 6  # drop_remainder


# ---- refusals and symbols ---------------------------------------------------------------------------------------------------------------------
def test_trainer_refusals_come_before_the_device():
    from mindaudio_amd.models import WaveGrad, WaveGradTrainer

    model = WaveGrad(T.TINY)
    with pytest.raises(TypeError):
        WaveGradTrainer(torch.nn.Linear(2, 2), 1e-3)
    with pytest.raises(ValueError):
        WaveGradTrainer(model, 1e-3, operands="fp8")
    with pytest.raises(ValueError):
        WaveGradTrainer(model, 0.0)
    with pytest.raises(ValueError):
        WaveGradTrainer(model, 1e-3, loss_scale=0.5)
    tr = WaveGradTrainer(model, 1e-3)
    audio, spec, level = torch.zeros(2, 60), torch.zeros(2, 8, 2), torch.tensor([0.5, 0.5])
    with pytest.raises(ValueError, match="HIP device"):
        tr.loss_and_grads(audio, level, audio, spec)  # CPU tensors
    with pytest.raises(ValueError):
        tr.loss_and_grads(audio[0], level, audio, spec)  # rank
    with pytest.raises(ValueError, match="hop_samples"):
        tr.loss_and_grads(torch.zeros(2, 61), level, torch.zeros(2, 61), spec)  # T != hop * frames
    with pytest.raises(ValueError):
        tr.step(audio, level, audio, torch.zeros(2, 7, 2))  # n_mels
    assert tr.params is None and tr.steps == 0  # nothing was bound


def test_noise_of_another_shape_is_refused_before_the_device(monkeypatch):
    """The model's own checks pass (they are stubbed to do so for CPU tensors); the trainer's noise checks come next, still in front of
    every device call."""
    from mindaudio_amd.models import WaveGrad, WaveGradTrainer

    model = WaveGrad(T.TINY)
    tr = WaveGradTrainer(model, 1e-3)
    monkeypatch.setattr(model, "_check_inputs", lambda audio, spec: (audio.shape[0], audio.shape[1], spec.shape[2]))
    audio, spec, level = torch.zeros(2, 60), torch.zeros(2, 8, 2), torch.tensor([0.5, 0.5])
    with pytest.raises(ValueError, match="noise must be a"):
        tr.loss_and_grads(audio, level, torch.zeros(2, 59), spec)
    with pytest.raises(ValueError, match="noise must be on"):
        tr.loss_and_grads(audio, level, torch.zeros(2, 60), spec)
    with pytest.raises(ValueError, match="noise must be a"):
        tr.step(audio, level, None, spec)
    assert tr.params is None


def test_script_refusals():
    from mindaudio_amd.wavegrad import train as script

    with pytest.raises(NotImplementedError, match="is_distributed"):
        script.main(["--is_distributed", "True", "--config", "/nonexistent.yaml"])  # before the config is even read
    with pytest.raises(NotImplementedError):
        script.train(None, is_distributed=True)
    with pytest.raises(SystemExit):
        script.main(["--operands", "fp8"])


def test_new_symbols_are_bound():
    from mindaudio_amd import _lib

    for sym in ("ma_wavegrad_l1_last_bwd_f32", "ma_wavegrad_pack_bwd_f32", "ma_wavegrad_init_conv_bwd_f32", "ma_wavegrad_sumsq_f64",
                "ma_wavegrad_clip_adam_f32", "ma_wavegrad_weights_bf16", "ma_wavegrad_pack_f32", "ma_wavegrad_last_bwd_parts",
                "ma_wavegrad_init_bwd_parts", "ma_wavegrad_sumsq_parts"):
        assert sym in _lib.PROTOTYPES, sym
    assert _lib.ABI_VERSION == 4
    assert ctypes_sizeof_weight_item() == 56


def ctypes_sizeof_weight_item():
    import ctypes

    from mindaudio_amd import _lib

    return ctypes.sizeof(_lib.WaveGradWeightItem)


def test_host_only_entry_points_and_argument_checks():
    """Everything that returns before the first HIP call: the partial counts and the refusals of every new entry."""
    from mindaudio_amd import _build, _lib

    _build.build()
    lib = _lib.load()
    assert lib.ma_wavegrad_last_bwd_parts(2, 65) == 4 and lib.ma_wavegrad_last_bwd_parts(32, 9000) == 32 * 141
    assert lib.ma_wavegrad_init_bwd_parts(3, 257) == 6 and lib.ma_wavegrad_last_bwd_parts(0, 5) == _lib.MA_ERR_INVALID_ARG
    assert lib.ma_wavegrad_sumsq_parts(1000) == 1 and lib.ma_wavegrad_sumsq_parts(17907080) == 1024
    assert lib.ma_wavegrad_sumsq_parts(3 * 4096 * 4 + 8) == 4
    a = 4096  # an aligned, never dereferenced address
    bad = _lib.MA_ERR_INVALID_ARG
    assert lib.ma_wavegrad_l1_last_bwd_f32(a, a, a, 2, 8, 8, a, 4, 1.0, a, a, a, 40, a, a, None) == bad              # even taps
    assert lib.ma_wavegrad_l1_last_bwd_f32(a, a, a, 2, 8, 8, a, 3, 1.0, a, a, a, 24, a, a, None) == bad              # pstride < taps C + 1
    assert lib.ma_wavegrad_l1_last_bwd_f32(a, a, a + 4, 2, 8, 8, a, 3, 1.0, a, a, a, 32, a, a, None) == bad          # misaligned x
    assert lib.ma_wavegrad_l1_last_bwd_f32(a, a, a, 2, 8, 6, a, 3, 1.0, a, a, a, 32, a, a, None) == _lib.MA_ERR_UNSUPPORTED   # C % 4
    assert lib.ma_wavegrad_pack_bwd_f32(None, 0, a, 2, 4, 1, 8, None, 0, 1.0, 1.0, None, 0.0, a, 0, None, 0, 0, None) == bad  # no gradient
    assert lib.ma_wavegrad_pack_bwd_f32(a, 4, a, 2, 4, 1, 8, None, 0, 1.0, 1.0, None, 0.0, a, 0, None, 0, 0, None) == bad    # ld_dop < C
    assert lib.ma_wavegrad_pack_bwd_f32(a, 8, a, 2, 4, 1, 8, None, 0, 1.0, 1.0, None, 0.0, a, 0, a, 16, 0, None) == bad     # dfilm without film
    assert lib.ma_wavegrad_init_conv_bwd_f32(a, a, 2, 8, 9, 8, a, None) == _lib.MA_ERR_UNSUPPORTED                           # taps > 7
    assert lib.ma_wavegrad_sumsq_f64(a, 6, a, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_wavegrad_clip_adam_f32(a, a, a, a, 8, a, 1, 0.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, a, a, None) == bad            # loss scale 0
    assert lib.ma_wavegrad_clip_adam_f32(a, a, a, a, 8, a, 2000, 1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8, a, a, None) == _lib.MA_ERR_UNSUPPORTED
    assert lib.ma_wavegrad_weights_bf16(None, a, 1, None) == bad
    assert lib.ma_wavegrad_pack_f32(a, 2, 4, 1, 6, 0, None, 0, None, 0, 1.0, 1.0, a, None, 0.0, None) == _lib.MA_ERR_UNSUPPORTED


def test_trainer_binds_views_and_keeps_reference_names():
    """Binding needs no device: the model's parameters become (out, in, k) views of the flat masters kept in operand order, and
    state_dict() returns the values that went in."""
    from mindaudio_amd.models import WaveGrad, WaveGradTrainer
    from mindaudio_amd.train.flat import stored_last_first

    c = T.case("tiny_b2")
    model = WaveGrad(c["hps"])
    model.load_state_dict(c["state"])
    tr = WaveGradTrainer(model, 1e-3, operands="f32")
    tr._bind(torch.device("cpu"))
    sd = tr.state_dict()
    shapes = W.param_shapes(c["hps"])
    assert all(torch.equal(sd[k], c["state"][k]) and tuple(sd["moment1." + k].shape) == tuple(shapes[k]) for k in shapes)
    off, shape, n = tr.params.index["UBlock.0.block2_a.weight"]
    w = c["state"]["UBlock.0.block2_a.weight"]
    assert torch.equal(tr.params.master[off:off + n].view(shape[0], shape[2], shape[1]), w.permute(0, 2, 1))  # (N, taps, C)
    off, shape, n = tr.params.index["DBlock.0.weight"]
    assert tr.params._layout["DBlock.0.weight"] is stored_last_first and torch.equal(tr.params.master[off:off + n].view(shape[2], shape[0]), c["state"]["DBlock.0.weight"][:, 0, :].t())
    model.last_conv.weight.data.mul_(2.0)  # the parameter IS the master
    off, _, n = tr.params.index["last_conv.weight"]
    assert torch.equal(tr.params.master[off:off + n].view(3, -1), 2.0 * c["state"]["last_conv.weight"][0].t())
    assert tr.params.size % 8 == 0 and all(s[0] % 8 == 0 for s in tr.params.index.values())
