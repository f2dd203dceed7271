"""GPU: models.DeepSpeech2Trainer on the small model of deepspeech2_cases.model_case (2 layers, H 64, B 3, T 40 -> 20 LSTM steps)
against float64 restatements of everything behind the frozen front end: the recurrent stack, fc, NetWithCTCLoss and nn.Adam.

  exact      torch.autograd in float64 over RNN + fc + log_softmax + F.ctc_loss, nothing rounded, on the device's own LSTM input.
  rounded    the closed forms of lstm_train_cases / deepspeech2_cases with bf16 at the device's rounding points (x, W_ih, W_hh, the
             fed-back h, dgates, the fc operands, dlogits).  S = relrms(rounded, exact) per parameter; the device is allowed 2 S."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deepspeech2_cases as C
import lstm_train_cases as L

pytestmark = pytest.mark.gpu

LENGTHS = np.array([40, 34, 27], np.int32)
TARGETS = [[1, 2, 2, 27, 5, 9], [20, 8, 5, 27, 27], [3, 1, 20]]  # with adjacent repeats, which need a blank frame each
LOSS_SCALE, LR, EPS = 1024.0, 3e-4, 1e-5  # the yaml's


def _targets():
    ylens = np.array([len(t) for t in TARGETS], np.int32)
    ys = np.full((len(TARGETS), 8), 28, np.int32)  # padded with the blank id, as the reference pads; the lengths say where rows end
    for b, t in enumerate(TARGETS):
        ys[b, :len(t)] = t
    return ys, ylens


def _model(cfg, state):
    from mindaudio_amd.models import DeepSpeechModel

    m = DeepSpeechModel(batch_size=cfg["B"], labels=C.LABELS, rnn_hidden_size=cfg["H"], nb_layers=cfg["layers"],
                        audio_conf=dict(sample_rate=cfg["sample_rate"], window_size=cfg["window_size"]))
    m.load_weights(state)
    return m.cuda().eval()


def _trainer(seed=0, **kw):
    from mindaudio_amd.models import DeepSpeech2Trainer

    cfg, state, x, _, _ = C.model_case("small", seed)
    model = _model(cfg, state)
    return cfg, state, x, model, DeepSpeech2Trainer(model, LR, kw.pop("eps", EPS), loss_scale=LOSS_SCALE, **kw)


def _trained_names(cfg):
    return [n for n in C.param_shapes(**cfg) if not n.startswith("conv.")]


@pytest.fixture(scope="module")
def run():
    """One loss_and_grads on the small case with everything the tests below compare: computed once, left unchanged."""
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    cfg, state, x, model, tr = _trainer()
    ys, ylens = _targets()
    out_len = C.get_seq_lens(LENGTHS)
    repeats = np.array([sum(a == b for a, b in zip(t, t[1:])) for t in TARGETS])
    assert np.all(ylens + repeats <= out_len), "an infeasible target: its loss would be infinite"
    want_logits, _ = model(x, LENGTHS)
    want_logits = want_logits.clone()
    loss = tr.loss_and_grads(x, LENGTHS, ys, ylens)
    grads = {k: v.double().cpu().numpy() / LOSS_SCALE for k, v in tr.gradients().items()}
    xin = model.frontend(torch.from_numpy(x).cuda()).double().cpu().numpy()  # (T1, B, Kpad), feature f * 32 + c
    F2 = model.F2
    xin = xin[:, :, :32 * F2].reshape(xin.shape[0], cfg["B"], F2, 32).transpose(0, 1, 3, 2).reshape(xin.shape[0], cfg["B"], 32 * F2)
    return dict(cfg=cfg, state=state, x=x, model=model, tr=tr, ys=ys, ylens=ylens, out_len=out_len, loss=loss, grads=grads, xin=xin,
                logits=tr.logits.clone(), want_logits=want_logits)


def _ctc(logits, ys, out_len, ylens):
    """logits (T, B, C) float64 tensor -> the mean over the batch of the CTC losses, blank last."""
    lp = torch.log_softmax(logits, -1)
    per = F.ctc_loss(lp, torch.from_numpy(ys).long(), torch.from_numpy(out_len).long(), torch.from_numpy(ylens).long(),
                     blank=logits.shape[-1] - 1, reduction="none", zero_infinity=True)
    return per.sum() / logits.shape[1]


def _exact(run):
    """float64 autograd over RNN + fc + CTC on xin (reference feature order) -> (loss, {name: gradient})"""
    f64, cfg = torch.float64, run["cfg"]
    p = {n: torch.tensor(np.asarray(run["state"][n], np.float64), dtype=f64, requires_grad=True) for n in _trained_names(cfg)}
    h = torch.tensor(run["xin"], dtype=f64)
    T, B, H = h.shape[0], cfg["B"], cfg["H"]
    for k in range(cfg["layers"]):
        out = [torch.zeros((B, H), dtype=f64) for _ in range(T)]
        for d, suffix in enumerate(("", "_reverse")):
            w_ih, w_hh, b_ih, b_hh = (p["RNN.lstms.%d.%s_l0%s" % (k, n, suffix)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            hh, c = torch.zeros((B, H), dtype=f64), torch.zeros((B, H), dtype=f64)
            for s in range(T):
                t = T - 1 - s if d else s
                i, f, g, o = (h[t] @ w_ih.T + b_ih + hh @ w_hh.T + b_hh).chunk(4, dim=1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                hh = torch.sigmoid(o) * torch.tanh(c)
                out[t] = out[t] + hh
        h = torch.stack(out)
    loss = _ctc(h @ p["fc.module.weight"].T, run["ys"], run["out_len"], run["ylens"])
    loss.backward()
    return float(loss.detach()), {n: v.grad.numpy() for n, v in p.items()}


def _rounded(run):
    """The same step in closed form with the device's rounding points -> {name: gradient}"""
    cfg, state, r = run["cfg"], run["state"], C.bf16_round
    layers = [C.layer_of(state, k) for k in range(cfg["layers"])]
    hs = [run["xin"]]
    for layer in layers:
        hs.append(C.lstm_bidir(hs[-1], layer, rounding=True)[0])
    wfc = r(np.asarray(state["fc.module.weight"], np.float64))
    logits = torch.tensor(r(hs[-1]) @ wfc.T, dtype=torch.float64, requires_grad=True)
    _ctc(logits, run["ys"], run["out_len"], run["ylens"]).backward()
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
    return grads


def test_logits_have_the_bits_of_model_forward(run):
    assert run["logits"].shape == run["want_logits"].shape
    assert torch.equal(run["logits"].view(torch.int32), run["want_logits"].contiguous().view(torch.int32))


def test_loss_matches_float64(run):
    """On the device's own logits, so that only the loss's arithmetic enters; the bound is test_train_kernels_gpu.test_ctc_loss_grad's."""
    want = float(_ctc(run["logits"].double().cpu(), run["ys"], run["out_len"], run["ylens"]))
    print("loss %.6f, float64 %.6f, relative difference %.2e" % (run["loss"], want, abs(run["loss"] - want) / abs(want)))
    assert np.isfinite(want) and abs(run["loss"] - want) < 1e-4 * abs(want)


def test_gradients_against_float64_autograd(run):
    loss, exact = _exact(run)
    rounded = _rounded(run)
    assert abs(run["loss"] - loss) <= 3e-2 * abs(loss)  # (the whole forward's rounding: a coarse check that the two are the same problem)
    assert sorted(run["grads"]) == sorted(exact) == sorted(_trained_names(run["cfg"]))
    for name in sorted(exact):
        got, want = run["grads"][name], exact[name]
        assert got.shape == want.shape, name
        S, e = C.relrms(rounded[name], want), C.relrms(got, want)
        cos = float((got * want).sum() / np.sqrt((got * got).sum() * (want * want).sum()))
        print("%-34s relrms %.3e, rounding-only S %.3e, ratio %.2f, cosine %.6f" % (name, e, S, e / S, cos))
        assert 0 < S < 5e-2 and e <= 2 * S, name
    for k in range(run["cfg"]["layers"]):
        for suffix in ("", "_reverse"):
            assert np.array_equal(run["grads"]["RNN.lstms.%d.bias_ih_l0%s" % (k, suffix)], run["grads"]["RNN.lstms.%d.bias_hh_l0%s" % (k, suffix)])


def test_layer0_weight_ih_gradient_is_in_the_reference_column_order(run):
    """An LSTM input that is non-zero in ONE channel c0 only: in the reference's order the gradient's columns c0 * F2 .. c0 * F2 + F2 - 1
    are the only non-zero ones, exactly."""
    from mindaudio_amd import ops
    from mindaudio_amd.models._lstm import ceil64
    from mindaudio_amd.models.deepspeech2_train import unpermute_wih_columns

    model, tr = run["model"], run["tr"]
    F2, H, c0, T, B = model.F2, model.hidden_size, 7, 4, 3
    Lyr = model._prepared["layers"][0]
    x = torch.zeros((T, B, F2, 32), dtype=torch.bfloat16, device="cuda")
    x[:, :, :, c0] = torch.randn((T, B, F2), device="cuda").to(torch.bfloat16)
    xin = torch.zeros((T, B, ceil64(32 * F2)), dtype=torch.bfloat16, device="cuda")
    xin[:, :, :32 * F2] = x.view(T, B, 32 * F2)
    _, _, tape = ops.lstm_bidir_train(xin, Lyr)
    res = ops.lstm_bidir_backward(torch.randn((T, B, H), device="cuda"), tape, Lyr, need_dx=False)
    for d in (0, 1):
        dw = unpermute_wih_columns(res["dw_ih"][d][:, :32 * F2], 32, F2).cpu().numpy()
        hot = np.zeros(32 * F2, bool)
        hot[c0 * F2:(c0 + 1) * F2] = True
        assert not np.any(dw[:, ~hot]) and np.all(np.abs(dw[:, hot]).max(0) > 0)
    assert tr.gradients()["RNN.lstms.0.weight_ih_l0"].shape == (4 * H, 32 * F2)


def _adam_f64(p, m, v, g, t, lr, eps, inv_scale):
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    g = g * inv_scale
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    delta = lr_t * m / (np.sqrt(v) + eps)
    return p - delta, m, v, delta, lr_t


def test_three_steps_against_float64_adam():
    """Each step: the float64 update of the parameters and moments before it with the step's own gradient, the gradient divided by
    loss_scale * optimizer_loss_scale.  Bounds, u = 2^-24 per float32 operation, g' = g / scale^2 (one rounding):
      m' = b1 m + (1 - b1) g'      err_m <= 4 u (|b1 m| + |(1 - b1) g'|)   (the constant, two products, the sum; the terms may cancel)
      v' = b2 v + (1 - b2) g'^2    err_v <= 6 u v'                          (all terms are non-negative)
      delta = lr_t m' / (sqrt(v') + eps)   lr_t err_m / (sqrt(v') + eps) + 10 u |delta|   (sqrt(v') to 3 u + its own rounding, lr_t as a
                                           float32, the sum, the quotient, the product)
      p' = p - delta               u |p'| more."""
    eps = 1e-6  # (larger than the scaled gradients' sqrt(v), so that the second division by the scale shows)
    cfg, state, x, model, tr = _trainer(eps=eps)
    ys, ylens = _targets()
    u, inv = 2.0 ** -24, 1.0 / (LOSS_SCALE * LOSS_SCALE)
    single_division_differs = False
    for t in (1, 2, 3):
        names = list(tr.params.index) if tr.params is not None else None
        before = None if names is None else {n: [tr.params._view(b, n).double().cpu().numpy() for b in (tr.params.master, tr.params.moment1, tr.params.moment2)] for n in names}
        if before is None:  # the first step binds the parameters: they are the model's, the moments zero
            before = {n: [np.asarray(state[n], np.float64), 0.0, 0.0] for n in [k for k in state if not k.startswith("conv.")]}
        loss, overflow = tr.step(x, LENGTHS, ys, ylens)
        assert np.isfinite(loss) and not overflow and tr.steps == t
        for n, (p0, m0, v0) in before.items():
            g = tr.gradients()[n].double().cpu().numpy()
            p1, m1, v1, delta, lr_t = _adam_f64(p0, m0, v0, g, t, LR, eps, inv)
            got_p, got_m, got_v = (tr.params._view(b, n).double().cpu().numpy() for b in (tr.params.master, tr.params.moment1, tr.params.moment2))
            b1 = float(np.float32(0.9))
            tiny = 2.0 ** -126  # a float32 result below the smallest normal number may be flushed to zero
            err_m = 4 * u * (np.abs(b1 * m0) + np.abs((1 - b1) * g * inv)) + tiny
            bound_p = u * np.abs(p1) + lr_t * err_m / (np.sqrt(v1) + eps) + (10 * u + 2.0 ** -63 / eps) * np.abs(delta)
            assert np.all(np.abs(got_m - m1) <= err_m), n
            assert np.all(np.abs(got_v - v1) <= 6 * u * v1 + tiny), n
            assert np.all(np.abs(got_p - p1) <= bound_p), n
            wrong = _adam_f64(p0, m0 * LOSS_SCALE, v0 * LOSS_SCALE ** 2, g, t, LR, eps, 1.0 / LOSS_SCALE)[0]
            single_division_differs |= bool(np.any(np.abs(got_p - wrong) > 100 * bound_p))
    assert single_division_differs  # dividing once only is a different optimizer at this eps
    # the model computes with the updated weights
    logits, _ = model(x, LENGTHS)
    assert C.relrms(logits.cpu().numpy(), C.model_case("small")[3]) > 1e-4


def test_non_finite_input_sets_overflow_and_keeps_every_bit():
    cfg, state, x, model, tr = _trainer()
    ys, ylens = _targets()
    tr.step(x, LENGTHS, ys, ylens)
    keep = [b.clone() for b in (tr.params.master, tr.params.moment1, tr.params.moment2)]
    bad = x.copy()
    bad[1, 0, 3, 5] = np.nan  # (an infinite sample would only saturate the frozen front end's tanh: NaN goes through)
    _, overflow = tr.step(bad, LENGTHS, ys, ylens)
    assert overflow and tr.steps == 1
    for a, b in zip(keep, (tr.params.master, tr.params.moment1, tr.params.moment2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    loss, overflow = tr.step(x, LENGTHS, ys, ylens)  # and the next clean step goes through
    assert np.isfinite(loss) and not overflow and tr.steps == 2


def test_state_dict_round_trip_and_the_next_step_is_bit_equal():
    from mindaudio_amd.models import DeepSpeech2Trainer

    cfg, state, x, model, tr = _trainer()
    ys, ylens = _targets()
    tr.step(x, LENGTHS, ys, ylens)
    sd = tr.state_dict()
    names = _trained_names(cfg)
    assert int(sd["steps"]) == 1 and all("moment1." + n in sd and "moment2." + n in sd for n in names)
    assert not any(k.startswith("moment1.conv.") for k in sd)
    other = DeepSpeech2Trainer(_model(cfg, C.make_state(cfg, 77)), LR, EPS, loss_scale=LOSS_SCALE)
    other.load_state_dict(sd)
    a, b = tr.step(x, LENGTHS, ys, ylens), other.step(x, LENGTHS, ys, ylens)
    assert a == b and other.steps == 2
    for u, v in zip((tr.params.master, tr.params.moment1, tr.params.moment2), (other.params.master, other.params.moment1, other.params.moment2)):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_refusals():
    cfg, state, x, model, tr = _trainer()
    long_ys = np.ones((3, 224), np.int32)
    with pytest.raises(ValueError):
        tr.loss_and_grads(x, LENGTHS, long_ys, np.array([224, 3, 3]))
    tr.loss_and_grads(x, LENGTHS, long_ys, np.array([3, 3, 3]))  # (a wide array with short rows is fine)
    from mindaudio_amd.models import DeepSpeech2Trainer

    with pytest.raises(NotImplementedError):
        DeepSpeech2Trainer(model, LR, EPS, train_conv=True)


def test_train_script_end_to_end(tmp_path):
    """deepspeech2.train.train on one bin of two short utterances with the small geometry: seven steps, the checkpoint of step 5 under
    the reference's name, and a second run that starts from it (parameters, moments and Adam's step count) repeats steps 6 and 7."""
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
    lines = []
    losses = T.train(config, log=lines.append, max_steps=7)
    assert len(losses) == 7 and np.all(np.isfinite(losses))
    assert lines[0].startswith("epoch: 1 step: 1, loss is ") and lines[1].startswith("epoch: 2 step: 1, loss is ")  # one bin per epoch
    assert os.listdir(tmp_path / "ck") == ["DeepSpeech-5_1.ckpt"]
    raw = ckpt.read_mindspore_ckpt(str(tmp_path / "ck" / "DeepSpeech-5_1.ckpt"))
    assert "RNN.lstms.0.weight_ih_l0" in raw and "moment2.fc.module.weight" in raw and "conv.bn1.moving_mean" in raw
    assert int(raw["global_step"][0]) == 5
    config2 = dict(config, Pretrained_model=str(tmp_path / "ck" / "DeepSpeech-5_1.ckpt"),
                   CheckpointConfig=dict(config["CheckpointConfig"], ckpt_path=str(tmp_path / "ck2")))
    lines2 = []
    again = T.train(config2, log=lines2.append, max_steps=2)
    assert lines2[0] == "Successfully loading the pre-trained model"
    assert again == losses[5:7]  # the same parameters, moments and step count: the same bits
