"""GPU: ops.ds2_frontend_train / ops.ds2_frontend_backward (csrc/deepspeech2_train.hip and the products between its kernels) against the
float64 restatement of ds2_frontend_train_cases and torch.autograd, without the LSTM stack.

Shapes: deepspeech2_cases.SMALL (F 17, F1 9, F2 5, B 3, T 45 -> T1 23: odd, no multiple of any frames-per-workgroup count, the last
time taps outside the input) and YAML_GEOMETRY (F 161, F1 81, F2 41, B 2, T 40: a thread's third frequency slot partly empty, the
real 704- and 384-column runs).  u = 2^-24."""
import numpy as np
import pytest
import torch

import deepspeech2_cases as C
import ds2_frontend_train_cases as FE

pytestmark = pytest.mark.gpu
U = FE.U
CASES = ("small", "yaml-geometry")


def _model(cfg, state):
    from mindaudio_amd.models import DeepSpeechModel

    m = DeepSpeechModel(batch_size=cfg["B"], labels=C.LABELS, rnn_hidden_size=cfg["H"], nb_layers=cfg["layers"],
                        audio_conf=dict(sample_rate=cfg["sample_rate"], window_size=cfg["window_size"]))
    m.load_weights(state)
    return m.cuda().eval()


_RUNS = {}


def _run(name):
    """One forward and one backward on the device plus the float64 references: computed once per case, left unchanged."""
    if name in _RUNS:
        return _RUNS[name]
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    from mindaudio_amd import ops

    cfg, state, x, dout, _, rounded, _, fe, fr = FE.case(name)  # (shared with the CPU tests of the restatement)
    model = _model(cfg, state)
    xin, tape = ops.ds2_frontend_train(model, x)
    xin_dev = xin.double().cpu().numpy()
    act1_dev = tape.act1.double().cpu().numpy().reshape(tape.T1 + 10, tape.B, tape.Fpad, 32)
    dxin = torch.from_numpy(FE.to_device_xin(dout, tape.Kpad).astype(np.float32)).cuda()
    res = ops.ds2_frontend_backward(dxin, tape, keep=True)
    grads = {n: res[n].double().cpu().numpy() for n in FE.PARAMS}
    extra = {k: res[k].double().cpu().numpy() for k in ("dz1", "dact1")}
    _, exact, _ = FE.autograd(state, x, dout)
    _RUNS[name] = dict(cfg=cfg, state=state, x=x, dout=dout, model=model, tape=tape, xin=xin_dev, act1=act1_dev, dxin=dxin, grads=grads,
                       extra=extra, fe=fe, fr=fr, rounded=rounded, exact=exact,
                       y1=tape.y1.double().cpu().numpy(), y2=tape.y2.double().cpu().numpy(),
                       stats=[tape.stats1.double().cpu().numpy(), tape.stats2.double().cpu().numpy()],
                       moving=tape.moving.double().cpu().numpy())
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_batch_statistics_against_the_float64_moments_of_the_raw_output(name):
    """The device's (mean, biased variance) against the float64 moments of the device's OWN y1 / y2: |mean - mean64| <= 4 u mean|y|,
    |var - var64| <= 12 u E[y^2] (ds2_frontend_train_cases.stats_failures has the derivation); rstd = 1 / sqrt(var + eps) to 4 u."""
    r = _run(name)
    t = r["tape"]
    for y, st, axis in ((r["y1"], r["stats"][0], 3), (r["y2"].reshape(-1, t.F2, 32), r["stats"][1], 2)):
        mean, rstd, var = st[:32], st[32:64], st[64:]
        assert FE.stats_failures(mean, var, y, axis) == []
        assert np.all(np.abs(rstd - 1.0 / np.sqrt(var + FE.BN_EPS)) <= 4 * U * rstd)


@pytest.mark.parametrize("name", CASES)
def test_moving_statistics_of_one_forward(name):
    """moving = 0.9 old + 0.1 batch with the UNBIASED variance, within 4 u; the model's own vectors are not touched."""
    r = _run(name)
    t, s = r["tape"], r["state"]
    for i, (st, n) in enumerate(zip(r["stats"], (t.T1 * t.B * t.F1, t.T1 * t.B * t.F2))):
        old_m, old_v = (np.asarray(s["conv.bn%d.%s" % (i + 1, k)], np.float64) for k in ("moving_mean", "moving_variance"))
        want_m, want_v = 0.9 * old_m + 0.1 * st[:32], 0.9 * old_v + 0.1 * st[64:] * n / (n - 1)
        got_m, got_v = r["moving"][64 * i:64 * i + 32], r["moving"][64 * i + 32:64 * i + 64]
        assert np.all(np.abs(got_m - want_m) <= 4 * U * (np.abs(0.9 * old_m) + np.abs(0.1 * st[:32])))
        assert np.all(np.abs(got_v - want_v) <= 4 * U * want_v)
        biased = 0.9 * old_v + 0.1 * st[64:]
        assert np.all(np.abs(got_v - biased) > 4 * U * want_v)  # (the biased variance would be a different update)
        bn = getattr(r["model"].conv, "bn%d" % (i + 1))
        assert np.array_equal(bn.moving_mean.detach().cpu().numpy(), s["conv.bn%d.moving_mean" % (i + 1)])
        assert np.array_equal(bn.moving_variance.detach().cpu().numpy(), s["conv.bn%d.moving_variance" % (i + 1)])


@pytest.mark.parametrize("name", CASES)
def test_forward_against_the_rounding_only_restatement(name):
    r = _run(name)
    t = r["tape"]
    exact, rounded = FE.to_device_xin(r["fe"]["out"], t.Kpad), FE.to_device_xin(r["fr"]["out"], t.Kpad)
    S = C.relrms(rounded, exact)
    e_r, e_x = C.relrms(r["xin"], rounded), C.relrms(r["xin"], exact)
    print("%s xin: S %.3e, device against rounding-only %.3e, against exact %.3e" % (name, S, e_r, e_x))
    assert 0 < S < 5e-2 and e_r <= 2 * S and e_x <= 2 * S
    # the activation between the stages, at its place in the image
    a1 = FE.from_channel_last(r["act1"][5:5 + t.T1, :, 10:10 + t.F1, :])
    S1 = C.relrms(r["fr"]["act1"], r["fe"]["act1"])
    assert C.relrms(a1, r["fr"]["act1"]) <= 2 * S1
    # what must stay exactly zero
    assert not np.any(r["xin"][:, :, 32 * t.F2:])
    assert not np.any(r["act1"][:5]) and not np.any(r["act1"][5 + t.T1:])
    assert not np.any(r["act1"][:, :, :10]) and not np.any(r["act1"][:, :, 10 + t.F1:])


@pytest.mark.parametrize("name", CASES)
def test_gradients_against_float64_autograd(name):
    r = _run(name)
    for n in FE.PARAMS:
        got, want = r["grads"][n], r["exact"][n]
        assert got.shape == want.shape, n
        S, e, cos = C.relrms(r["rounded"][n], want), C.relrms(got, want), FE.cosine(got, want)
        print("%-14s %-20s relrms %.3e, rounding-only S %.3e, ratio %.2f, cosine %.6f" % (name, n, e, S, e / S, cos))
        assert 0 < S < 5e-2 and e <= 2 * S and cos >= 0.99, n


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("fpw", [0, 2, 7])
def test_conv1_weight_gradient_alone(name, fpw):
    """An unrounded float32 dz1: |dW1 - dW1_64| <= (n_chain + n_join) u sum|dz1 x| per element; n_chain = frames per workgroup x F1 fused
    multiply-adds (the kernel's header), n_join = 2: the double join's own error is far below u, then one rounding."""
    from mindaudio_amd import _lib, ops

    r = _run(name)
    t = r["tape"]
    dz1 = np.random.RandomState(5).normal(0, 1, (t.T1, t.B, t.F1, 32)).astype(np.float32)
    got = ops.ds2_conv1_dw(t.x, torch.from_numpy(dz1).cuda(), fpw).double().cpu().numpy()
    z = FE.from_channel_last(dz1)
    want = FE.conv2d_backward(np.asarray(r["x"], np.float64), np.zeros((32, 1, 41, 11)), z, (2, 2), (20, 5))[1]
    terms = FE.conv1_dw_abs_terms(r["x"], z)
    frames = t.B * t.T1
    per = fpw or -(-frames // 1024)
    assert _lib.load().ma_ds2_conv1_dw_parts(t.B, t.T, fpw) == -(-frames // per)
    bound = (per * t.F1 + 2) * U * terms
    err = np.abs(got - want)
    print("%s fpw %d: worst error / bound %.3f" % (name, fpw, float((err[bound > 0] / bound[bound > 0]).max())))  # (a tap that never meets the input has bound 0)
    assert got.shape == want.shape and np.all(err <= bound)


@pytest.mark.parametrize("name,point", [("small", "interior"), ("small", "corner"), ("yaml-geometry", "interior"), ("yaml-geometry", "corner")])
def test_conv1_weight_gradient_routes_a_single_sample(name, point):
    """x is a single 1.0 at (b, f, t): dW1[c, kf, kt] = dz1[t1, b, f1, c] exactly where 2 f1 + kf - 20 = f and 2 t1 + kt - 5 = t, else 0."""
    from mindaudio_amd import ops

    r = _run(name)
    t = r["tape"]
    b, f, tt = (1, t.F // 2, t.T // 2 + 1) if point == "interior" else (t.B - 1, 0, t.T - 1)
    x = torch.zeros((t.B, 1, t.F, t.T), device="cuda")
    x[b, 0, f, tt] = 1.0
    dz1 = torch.from_numpy(np.random.RandomState(6).normal(0, 1, (t.T1, t.B, t.F1, 32)).astype(np.float32)).cuda()
    got = ops.ds2_conv1_dw(x, dz1, 2).cpu().numpy()
    want = np.zeros((32, 1, 41, 11), np.float32)
    z, hits = dz1.cpu().numpy(), 0
    for kf in range(41):
        for kt in range(11):
            f2, t2 = f + 20 - kf, tt + 5 - kt
            if f2 % 2 == 0 and t2 % 2 == 0 and 0 <= f2 // 2 < t.F1 and 0 <= t2 // 2 < t.T1:
                want[:, 0, kf, kt] = z[t2 // 2, b, f2 // 2, :]
                hits += 1
    assert hits > 0 and np.array_equal(got, want)


@pytest.mark.parametrize("name", CASES)
def test_batchnorm_backward_invariants(name):
    """Per channel sum dz vanishes within 16 u sum|dz|.  sum dz xhat does NOT vanish when eps > 0: with xhat = (y - mean) rstd and
    rstd = 1 / sqrt(var + eps), mean(xhat^2) = var / (var + eps), so sum dz xhat = gamma rstd^3 eps sum(dn xhat) exactly (that is
    d_gamma's sum).  That identity is held within 16 u sum|dz xhat|; the plain form's residue is printed beside it.  Both stages,
    float32 dz, xhat from the device's own statistics."""
    from mindaudio_amd import ops

    r = _run(name)
    t = r["tape"]
    rows = t.T1 * t.B
    dz2 = torch.empty((rows, t.F2 * 32), device="cuda")
    bs2 = ops.ds2_bn_tanh_backward(t.y2, r["dxin"].view(rows, t.Kpad), t.stats2, t.gamma2, t.beta2, dz2).double().cpu().numpy()
    bs1 = np.concatenate([r["grads"]["conv.bn1.beta"], r["grads"]["conv.bn1.gamma"]])
    for stage, y, dz, st, gamma, bs in ((1, r["y1"].reshape(-1, 32), r["extra"]["dz1"].reshape(-1, 32), r["stats"][0], t.gamma1, bs1),
                                        (2, r["y2"].reshape(-1, 32), dz2.double().cpu().numpy().reshape(-1, 32), r["stats"][1], t.gamma2, bs2)):
        xhat = (y - st[:32]) * st[32:64]
        g = gamma.detach().double().cpu().numpy()
        s0, a0 = dz.sum(0), np.abs(dz).sum(0)
        s1, a1 = (dz * xhat).sum(0), np.abs(dz * xhat).sum(0)
        resid = s1 - g * st[32:64] ** 3 * FE.BN_EPS * bs[32:64]
        print("%s stage %d: sum dz / bound %.3f, identity / bound %.3f, plain sum dz xhat / bound %.3f" % (
            name, stage, float((np.abs(s0) / (16 * U * a0)).max()), float((np.abs(resid) / (16 * U * a1)).max()),
            float((np.abs(s1) / (16 * U * a1)).max())))
        assert np.all(np.abs(s0) <= 16 * U * a0) and np.all(np.abs(resid) <= 16 * U * a1)


def test_two_runs_give_equal_bits():
    from mindaudio_amd import ops

    r = _run("small")
    xin, tape = ops.ds2_frontend_train(r["model"], r["x"])
    assert np.array_equal(xin.double().cpu().numpy(), r["xin"])
    assert torch.equal(tape.y1, r["tape"].y1) and torch.equal(tape.stats2, r["tape"].stats2) and torch.equal(tape.moving, r["tape"].moving)
    res = ops.ds2_frontend_backward(r["dxin"], tape)
    for n in FE.PARAMS:
        assert np.array_equal(res[n].double().cpu().numpy(), r["grads"][n]), n
