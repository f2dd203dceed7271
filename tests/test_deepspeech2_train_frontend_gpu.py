"""GPU: models.DeepSpeech2Trainer(frontend="trained") on the small model of deepspeech2_cases (2 layers, H 64, B 3, T 45 -> 23 LSTM
steps) against float64 restatements of the whole step: train-mode MaskConv, the recurrent stack, fc, NetWithCTCLoss and nn.Adam.

  exact      torch.autograd in float64 from x through conv1 + BatchNorm (batch statistics) + tanh, conv2 + BatchNorm + tanh, RNN, fc,
             log_softmax and F.ctc_loss, nothing rounded.
  rounded    the closed forms of ds2_frontend_train_cases / lstm_train_cases / deepspeech2_cases with bf16 at the device's rounding
             points.  S = relrms(rounded, exact) per parameter; the device is allowed 2 S.
The lengths, targets and optimizer settings are those of test_deepspeech2_train_gpu.py (copied: test files do not import each other)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deepspeech2_cases as C
import ds2_frontend_train_cases as FE
import lstm_train_cases as L

pytestmark = pytest.mark.gpu

LENGTHS = np.array([40, 34, 27], np.int32)
TARGETS = [[1, 2, 2, 27, 5, 9], [20, 8, 5, 27, 27], [3, 1, 20]]  # with adjacent repeats, which need a blank frame each
LOSS_SCALE, LR, EPS = 1024.0, 3e-4, 1e-5  # the yaml's
MOVING = ["conv.bn%d.%s" % (i, k) for i in (1, 2) for k in ("moving_mean", "moving_variance")]


def _targets():
    ylens = np.array([len(t) for t in TARGETS], np.int32)
    ys = np.full((len(TARGETS), 8), 28, np.int32)
    for b, t in enumerate(TARGETS):
        ys[b, :len(t)] = t
    return ys, ylens


def _model(cfg, state):
    from mindaudio_amd.models import DeepSpeechModel

    m = DeepSpeechModel(batch_size=cfg["B"], labels=C.LABELS, rnn_hidden_size=cfg["H"], nb_layers=cfg["layers"],
                        audio_conf=dict(sample_rate=cfg["sample_rate"], window_size=cfg["window_size"]))
    m.load_weights(state)
    return m.cuda().eval()


def _trainer(seed=0, frontend="trained", **kw):
    from mindaudio_amd.models import DeepSpeech2Trainer

    cfg, state, x, _, _ = C.model_case("small", seed)
    model = _model(cfg, state)
    return cfg, state, x, model, DeepSpeech2Trainer(model, LR, kw.pop("eps", EPS), loss_scale=LOSS_SCALE, frontend=frontend, **kw)


def _trained_names(cfg):
    return [n for n in C.param_shapes(**cfg) if not n.endswith(("moving_mean", "moving_variance"))]


def _ctc(logits, ys, out_len, ylens):
    lp = torch.log_softmax(logits, -1)
    per = F.ctc_loss(lp, torch.from_numpy(ys).long(), torch.from_numpy(out_len).long(), torch.from_numpy(ylens).long(),
                     blank=logits.shape[-1] - 1, reduction="none", zero_infinity=True)
    return per.sum() / logits.shape[1]


def _exact(cfg, state, x, ys, out_len, ylens):
    """float64 autograd over the whole network -> (loss, {name: gradient})"""
    f64 = torch.float64
    p, out, _ = FE.autograd_frontend(state, x)
    p.update({n: torch.tensor(np.asarray(state[n], np.float64), dtype=f64, requires_grad=True) for n in _trained_names(cfg) if n not in p})
    B, H = cfg["B"], cfg["H"]
    h = out.reshape(B, -1, out.shape[3]).permute(2, 0, 1)  # (T1, B, 32 F2), feature c * F2 + f (deepspeech2.py:259-261)
    T = h.shape[0]
    for k in range(cfg["layers"]):
        acc = [torch.zeros((B, H), dtype=f64) for _ in range(T)]
        for d, suffix in enumerate(("", "_reverse")):
            w_ih, w_hh, b_ih, b_hh = (p["RNN.lstms.%d.%s_l0%s" % (k, n, suffix)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            hh, c = torch.zeros((B, H), dtype=f64), torch.zeros((B, H), dtype=f64)
            for s in range(T):
                t = T - 1 - s if d else s
                i, f, g, o = (h[t] @ w_ih.T + b_ih + hh @ w_hh.T + b_hh).chunk(4, dim=1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                hh = torch.sigmoid(o) * torch.tanh(c)
                acc[t] = acc[t] + hh
        h = torch.stack(acc)
    loss = _ctc(h @ p["fc.module.weight"].T, ys, out_len, ylens)
    loss.backward()
    return float(loss.detach()), {n: v.grad.numpy() for n, v in p.items()}


def _rounded(cfg, state, x, ys, out_len, ylens):
    """The same step in closed form with the device's rounding points -> {name: gradient}"""
    r = C.bf16_round
    fr = FE.forward(state, x, rounding=True)
    layers = [C.layer_of(state, k) for k in range(cfg["layers"])]
    hs = [C.rnn_input(fr["out"])]
    for layer in layers:
        hs.append(C.lstm_bidir(hs[-1], layer, rounding=True)[0])
    wfc = r(np.asarray(state["fc.module.weight"], np.float64))
    logits = torch.tensor(r(hs[-1]) @ wfc.T, dtype=torch.float64, requires_grad=True)
    _ctc(logits, ys, out_len, ylens).backward()
    T, B, _ = hs[-1].shape
    dlog = r(logits.grad.numpy())
    grads = {"fc.module.weight": dlog.reshape(T * B, -1).T @ r(hs[-1]).reshape(T * B, -1)}
    dh = dlog @ wfc
    for k in range(cfg["layers"] - 1, -1, -1):
        res = L.layer_step(hs[k], layers[k], dh, rounding=True)
        for d, suffix in enumerate(("", "_reverse")):
            pre = "RNN.lstms.%d." % k
            grads[pre + "weight_ih_l0" + suffix], grads[pre + "weight_hh_l0" + suffix] = res["dw_ih"][d], res["dw_hh"][d]
            grads[pre + "bias_ih_l0" + suffix] = grads[pre + "bias_hh_l0" + suffix] = res["db"][d]
        dh = res["dx"]
    dout = dh.transpose(1, 2, 0).reshape(fr["out"].shape)  # (T1, B, c * F2 + f) -> (B, 32, F2, T1)
    fe = FE.backward(state, fr, dout)
    grads.update({n: fe[n] for n in FE.PARAMS})
    return grads


@pytest.fixture(scope="module")
def run():
    """One loss_and_grads on the small case with everything the tests below compare: computed once, left unchanged."""
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    cfg, state, x, model, tr = _trainer()
    ys, ylens = _targets()
    out_len = C.get_seq_lens(LENGTHS)
    eval_logits = model(x, LENGTHS)[0].clone()
    loss = tr.loss_and_grads(x, LENGTHS, ys, ylens)
    grads = {k: v.double().cpu().numpy() / LOSS_SCALE for k, v in tr.gradients().items()}
    moving = {n: dict(model.named_parameters())[n].detach().cpu().numpy().copy() for n in MOVING}
    return dict(cfg=cfg, state=state, x=x, model=model, tr=tr, ys=ys, ylens=ylens, out_len=out_len, loss=loss, grads=grads,
                logits=tr.logits.clone(), eval_logits=eval_logits, moving=moving, launches=dict(tr.launches))


def test_gradients_against_float64_autograd(run):
    cfg, state, x = run["cfg"], run["state"], run["x"]
    loss, exact = _exact(cfg, state, x, run["ys"], run["out_len"], run["ylens"])
    rounded = _rounded(cfg, state, x, run["ys"], run["out_len"], run["ylens"])
    assert abs(run["loss"] - loss) <= 3e-2 * abs(loss)
    assert sorted(run["grads"]) == sorted(exact) == sorted(_trained_names(cfg))
    for name in sorted(exact):
        got, want = run["grads"][name], exact[name]
        assert got.shape == want.shape, name
        S, e = C.relrms(rounded[name], want), C.relrms(got, want)
        print("%-34s relrms %.3e, rounding-only S %.3e, ratio %.2f, cosine %.6f" % (name, e, S, e / S, FE.cosine(got, want)))
        assert 0 < S < 5e-2 and e <= 2 * S, name


def test_forward_uses_batch_statistics_and_loss_and_grads_leaves_the_moving_ones(run):
    assert C.relrms(run["logits"].cpu().numpy(), run["eval_logits"].cpu().numpy()) > 1e-3  # (by design: not model.forward's logits)
    for n in MOVING:
        assert np.array_equal(run["moving"][n], np.asarray(run["state"][n], np.float32)), n
    m = run["model"]
    assert run["launches"]["frontend_conv2_dw"] == 2 * 11 * m.F2 and run["launches"]["frontend_conv2_dx"] == m.F1
    assert run["launches"]["frontend_batchnorm"] == 6 and run["launches"]["frontend_conv1_dw"] == 2


def _adam_f64(p, m, v, g, t, lr, eps, inv_scale):
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    g = g * inv_scale
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    delta = lr_t * m / (np.sqrt(v) + eps)
    return p - delta, m, v, delta, lr_t


def test_three_steps_against_float64_adam_and_the_moving_statistics():
    """The bounds of test_deepspeech2_train_gpu.test_three_steps_against_float64_adam, same formulae, over every entry of the flat
    store (the six new ones among them).  Then: the moving statistics have advanced, the model in eval mode computes with the new
    convolutions and statistics, and a fresh model loaded from the trainer's state gives the same bits."""
    eps = 1e-6
    cfg, state, x, model, tr = _trainer(eps=eps)
    ys, ylens = _targets()
    before_logits = model(x, LENGTHS)[0].clone()
    u, inv = 2.0 ** -24, 1.0 / (LOSS_SCALE * LOSS_SCALE)
    for t in (1, 2, 3):
        names = list(tr.params.index) if tr.params is not None else None
        before = None if names is None else {n: [tr.params._view(b, n).double().cpu().numpy() for b in (tr.params.master, tr.params.moment1, tr.params.moment2)] for n in names}
        if before is None:
            before = {n: [np.asarray(state[n], np.float64), 0.0, 0.0] for n in _trained_names(cfg)}
        moving0 = {n: dict(model.named_parameters())[n].detach().double().cpu().numpy().copy() for n in MOVING}
        loss, overflow = tr.step(x, LENGTHS, ys, ylens)
        assert np.isfinite(loss) and not overflow and tr.steps == t
        assert all(n in before for n in FE.PARAMS)
        for n, (p0, m0, v0) in before.items():
            g = tr.gradients()[n].double().cpu().numpy()
            p1, m1, v1, delta, lr_t = _adam_f64(p0, m0, v0, g, t, LR, eps, inv)
            got_p, got_m, got_v = (tr.params._view(b, n).double().cpu().numpy() for b in (tr.params.master, tr.params.moment1, tr.params.moment2))
            b1 = float(np.float32(0.9))
            tiny = 2.0 ** -126
            err_m = 4 * u * (np.abs(b1 * m0) + np.abs((1 - b1) * g * inv)) + tiny
            bound_p = u * np.abs(p1) + lr_t * err_m / (np.sqrt(v1) + eps) + (10 * u + 2.0 ** -63 / eps) * np.abs(delta)
            assert np.all(np.abs(got_m - m1) <= err_m), n
            assert np.all(np.abs(got_v - v1) <= 6 * u * v1 + tiny), n
            assert np.all(np.abs(got_p - p1) <= bound_p), n
        for n in MOVING:  # a committed step: every vector has moved, by a tenth of its distance to the batch's value
            now = dict(model.named_parameters())[n].detach().double().cpu().numpy()
            assert np.all(now != moving0[n]), n
    logits, _ = model(x, LENGTHS)
    assert C.relrms(logits.cpu().numpy(), before_logits.cpu().numpy()) > 1e-4
    sd = tr.state_dict()
    fresh = _model(cfg, C.make_state(cfg, 77))
    fresh.load_state_dict({k: sd[k] for k in fresh.state_dict()})
    again, _ = fresh.cuda().eval()(x, LENGTHS)
    assert torch.equal(again.contiguous().view(torch.int32), logits.contiguous().view(torch.int32))


def test_non_finite_input_sets_overflow_and_keeps_every_bit():
    cfg, state, x, model, tr = _trainer()
    ys, ylens = _targets()
    tr.step(x, LENGTHS, ys, ylens)
    params = dict(model.named_parameters())
    keep = [b.clone() for b in (tr.params.master, tr.params.moment1, tr.params.moment2)] + [params[n].detach().clone() for n in MOVING]
    bad = x.copy()
    bad[1, 0, 3, 5] = np.nan
    _, overflow = tr.step(bad, LENGTHS, ys, ylens)
    assert overflow and tr.steps == 1
    for a, b in zip(keep, [tr.params.master, tr.params.moment1, tr.params.moment2] + [params[n].detach() for n in MOVING]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    loss, overflow = tr.step(x, LENGTHS, ys, ylens)  # and the next clean step goes through
    assert np.isfinite(loss) and not overflow and tr.steps == 2
    assert not torch.equal(keep[3], params[MOVING[0]].detach())


def test_state_dict_round_trip_and_the_next_step_is_bit_equal():
    from mindaudio_amd.models import DeepSpeech2Trainer

    cfg, state, x, model, tr = _trainer()
    ys, ylens = _targets()
    tr.step(x, LENGTHS, ys, ylens)
    sd = tr.state_dict()
    assert int(sd["steps"]) == 1 and all("moment1." + n in sd and "moment2." + n in sd for n in _trained_names(cfg))
    assert "moment1.conv.conv1.weight" in sd and sd["moment1.conv.conv1.weight"].shape == (32, 1, 41, 11)
    other_model = _model(cfg, C.make_state(cfg, 77))
    other = DeepSpeech2Trainer(other_model, LR, EPS, loss_scale=LOSS_SCALE, frontend="trained")
    other.load_state_dict(sd)
    a, b = tr.step(x, LENGTHS, ys, ylens), other.step(x, LENGTHS, ys, ylens)
    assert a == b and other.steps == 2
    for u, v in zip((tr.params.master, tr.params.moment1, tr.params.moment2), (other.params.master, other.params.moment1, other.params.moment2)):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    for n in MOVING:
        assert torch.equal(dict(model.named_parameters())[n].detach(), dict(other_model.named_parameters())[n].detach()), n


def test_frozen_default_is_unchanged(run):
    cfg, state, x, model, tr = _trainer(frontend="frozen")
    ys, ylens = _targets()
    want, _ = model(x, LENGTHS)
    want = want.clone()
    tr.loss_and_grads(x, LENGTHS, ys, ylens)
    assert sorted(tr.gradients()) == sorted(n for n in _trained_names(cfg) if not n.startswith("conv."))
    assert torch.equal(tr.logits.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    assert not any(k.startswith("frontend_") for k in tr.launches)


def test_train_script_with_a_trained_front_end(tmp_path):
    import json

    from scipy.io import wavfile

    from mindaudio_amd.deepspeech2 import train as T
    from mindaudio_amd.utils import ckpt

    g = np.random.RandomState(2)
    samples = []
    for i, (n, text) in enumerate(((4000, "AB C"), (6000, "HELLO"))):
        wavfile.write(str(tmp_path / ("u%d.wav" % i)), 16000, (0.1 * g.normal(0, 1, n) * 32767).astype(np.int16))
        (tmp_path / ("u%d.txt" % i)).write_text(text + "\n")
        samples.append({"wav_path": str(tmp_path / ("u%d.wav" % i)), "transcript_path": "u%d.txt" % i})
    manifest = tmp_path / "train.json"
    manifest.write_text(json.dumps({"root_path": str(tmp_path), "samples": samples}))
    config = {"TrainingConfig": dict(epochs=9, batch_size=2, train_manifest=str(manifest)),
              "SpectConfig": dict(sample_rate=1600, window_size=0.02, window_stride=0.01, window="hamming"),
              "ModelConfig": dict(rnn_type="LSTM", hidden_size=64, hidden_layers=2),
              "OptimConfig": dict(learning_rate=3e-4, epsilon=1e-5, loss_scale=1024),
              "CheckpointConfig": dict(ckpt_file_name_prefix="DeepSpeech", ckpt_path=str(tmp_path / "ck"), keep_checkpoint_max=2),
              "Pretrained_model": "", "labels": C.LABELS}
    losses = T.train(config, log=lambda _line: None, max_steps=3, frontend="trained", save_checkpoint_steps=3)
    assert len(losses) == 3 and np.all(np.isfinite(losses))
    assert os.listdir(tmp_path / "ck") == ["DeepSpeech-3_1.ckpt"]
    raw = ckpt.read_mindspore_ckpt(str(tmp_path / "ck" / "DeepSpeech-3_1.ckpt"))
    assert "moment2.conv.conv2.weight" in raw and raw["moment2.conv.conv2.weight"].shape == (32, 32, 21, 11)
    assert np.any(raw["moment2.conv.conv2.weight"] != 0) and "conv.bn1.moving_mean" in raw
    # a run that resumes from such a checkpoint restores parameters, moving statistics, all moments and Adam's step count: its
    # first step repeats step 4 of the run that wrote it, bit for bit
    ck3 = dict(config["CheckpointConfig"], ckpt_path=str(tmp_path / "ck3"))
    longer = T.train(dict(config, CheckpointConfig=ck3), log=lambda _line: None, max_steps=4, frontend="trained", save_checkpoint_steps=3)
    config2 = dict(config, Pretrained_model=str(tmp_path / "ck3" / "DeepSpeech-3_1.ckpt"),
                   CheckpointConfig=dict(config["CheckpointConfig"], ckpt_path=str(tmp_path / "ck4")))
    resumed = T.train(config2, log=lambda _line: None, max_steps=1, frontend="trained")
    assert len(longer) == 4 and resumed == longer[3:4]
