"""GPU: the WaveGrad vocoder (csrc/wavegrad.hip, models/wavegrad.py, wavegrad/reverse.py, wavegrad/preprocess.py).

Kernels, each against float64 of the same float32 inputs, with bounds that follow from the arithmetic (u = 2^-24):
  init conv     |d| <= (k + 2) u (sum |x| |w| + |b|): k fused multiply-adds from the bias.  An all-zero utterance between two that end /
                begin with an impulse equals the bias exactly (no tap crosses an utterance); the row behind the output is untouched.
  pack          every real element within one bf16 ulp of max(|v|, 2^-10) of the float64 value (the bound of test_gln_apply_bf16:
                round-to-nearest is half an ulp, the float32 arithmetic in front of it is far below the other half except at zero
                crossings, which the floor covers); halo rows and pad columns exactly zero after a call on a NaN-filled buffer; guard
                rows untouched; the float32 side output within 2 u relative; slope 1 without FiLM on bf16 values is the identity.
  last conv     pred within (3 C + 4) u (sum |x| |w| + |b|); audio_out within |c1| (2 u |audio| + |c2| (bound_pred + 2 u |pred|)) +
                2 u |sigma noise| + u |result|; the isolation case as above.
Model: S = relrms(bf16 restatement, float64 restatement) of tests/wavegrad_cases.py is computed here on the CPU, 5e-4 <= S <= 3e-2;
the device must be within 2 S of the float64 restatement (the device rounds where the bf16 restatement rounds, independently: sqrt(2)
S; the rest covers float32 accumulation order).  The loop the same way with S_loop, 1e-4 <= S_loop <= 3e-2.

Measured (S on the CPU of the GPU machine, then the device on an MI355X, 2026-10-20; the weights are make_state(hps, 1)):
  small, level 0.05   S 2.11e-3  device 2.11e-3      small, level 0.999  S 2.67e-3  device 2.73e-3
  yaml,  level 0.05   S 5.33e-3  device 5.33e-3      yaml,  level 0.999  S 5.21e-3  device 5.17e-3
  six-step loop       S_loop 5.86e-4  device 5.89e-4
(S moves in its third digit between machines with the order of the float64 sums inside the bf16 restatement's convolutions: 2.09e-3
and 2.75e-3 for the small model on another CPU.)  With N(0, 1 / fan_in) weights instead of the reference's initialisation the loop is
expansive and S_loop is 5e-2, outside its window: see wavegrad_cases.make_state."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import wavegrad_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LEVELS = (0.05, 0.999)
GEOMETRIES = {"small": (C.SMALL, C.SMALL_SHAPE), "yaml": (C.YAML, C.YAML_SHAPE)}


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def lib(torch):
    from mindaudio_amd import _host, _lib

    _host.require_gpu()
    return _lib.load()


def _ok(rc):
    assert rc == 0, rc


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ---- init conv ------------------------------------------------------------------------------------------------------------------------------
def _init_conv(torch, lib, audio, w, b):
    B, T = audio.shape
    C0, k = w.shape
    out = torch.full((B * T + 1, C0), float("nan"), device="cuda")  # one guard row behind the output
    ad, wt, bd = audio.cuda(), w.t().contiguous().cuda(), b.cuda()
    _ok(lib.ma_wavegrad_init_conv_f32(ad.data_ptr(), B, T, wt.data_ptr(), bd.data_ptr(), k, C0, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[-1]).all()), "the guard row was written"
    return out[:-1].cpu().view(B, T, C0)


@pytest.mark.parametrize("B,T,C0,k", [(3, 61, 32, 5), (2, 3, 32, 5), (2, 64, 64, 3)])
def test_init_conv(torch, lib, B, T, C0, k):
    g = torch.Generator().manual_seed(B * 1000 + T)
    audio, w, b = torch.randn((B, T), generator=g), torch.randn((C0, k), generator=g), torch.randn((C0,), generator=g)
    got = _init_conv(torch, lib, audio, w, b).double()
    F = torch.nn.functional
    want = F.conv1d(audio.double()[:, None], w.double()[:, None], b.double(), padding=k // 2).transpose(1, 2)
    mag = F.conv1d(audio.double().abs()[:, None], w.double().abs()[:, None], b.double().abs(), padding=k // 2).transpose(1, 2)
    ratio = ((got - want).abs() / ((k + 2) * U * mag)).max()
    assert float(ratio) <= 1.0, float(ratio)


def test_init_conv_never_reads_the_neighbouring_utterance(torch, lib):
    T, C0, k = 61, 32, 5
    g = torch.Generator().manual_seed(3)
    audio = torch.zeros((3, T))
    audio[0, -1], audio[2, 0] = 1000.0, -1000.0
    w, b = torch.randn((C0, k), generator=g), torch.randn((C0,), generator=g)
    got = _init_conv(torch, lib, audio, w, b)
    assert bool((got[1] == b[None, :]).all())
    assert bool((got[0, -1] != b).any()) and bool((got[2, 0] != b).any())


# ---- pack -----------------------------------------------------------------------------------------------------------------------------------
PACK_CASES = [  # C, T_in, f, film, enc, slope, halo
    (32, 5, 1, False, False, 1.0, 8), (32, 40, 2, False, True, 0.2, 8), (32, 5, 3, True, False, 0.2, 0), (64, 40, 1, True, True, 0.2, 8),
    (64, 5, 5, False, False, 0.2, 8), (64, 5, 2, True, False, 1.0, 0), (128, 40, 3, False, False, 0.2, 8), (128, 5, 5, True, True, 0.2, 8),
    (128, 40, 1, False, True, 1.0, 0), (128, 5, 2, True, False, 0.2, 8), (64, 40, 3, True, True, 1.0, 0), (32, 5, 5, True, True, 0.2, 8),
]


def _pack(torch, lib, x, f, Cpad, halo, film, ld_film, enc, ld_enc, slope, mul, want_res, res_mul, want_out=True):
    B, T_in, Cc = x.shape
    T = T_in * f
    guard = 2
    out = res = None
    if want_out:
        out = torch.full((B * (T + 2 * halo) + guard, Cpad), float("nan"), dtype=torch.bfloat16, device="cuda")
    if want_res:
        res = torch.full((B * T + guard, Cc), float("nan"), device="cuda")
    xd = x.cuda()
    fd = film.cuda() if film is not None else None
    ed = enc.cuda() if enc is not None else None
    _ok(lib.ma_wavegrad_pack_bf16(xd.data_ptr(), B, T_in, f, Cc, Cpad, halo, _ptr(fd), ld_film, _ptr(ed), ld_enc, slope, mul, _ptr(out),
                                  _ptr(res), res_mul, None))
    torch.cuda.synchronize()
    if out is not None:
        assert bool(torch.isnan(out[-guard:].float()).all()), "guard rows behind the operand buffer were written"
        out = out[:-guard].cpu().view(B, T + 2 * halo, Cpad)
    if res is not None:
        assert bool(torch.isnan(res[-guard:]).all()), "guard rows behind the side output were written"
        res = res[:-guard].cpu().view(B, T, Cc)
    return out, res


@pytest.mark.parametrize("Cc,T_in,f,film,enc,slope,halo", PACK_CASES)
def test_pack(torch, lib, Cc, T_in, f, film, enc, slope, halo):
    B, T, Cpad = 2, T_in * f, (Cc + 63) // 64 * 64
    g = torch.Generator().manual_seed(Cc * 100 + T_in * 10 + f)
    x = torch.randn((B, T_in, Cc), generator=g)
    ld_film = 2 * Cc + 8  # its own row stride
    fm = torch.randn((B * T, ld_film), generator=g) if film else None
    en = torch.randn((B, Cc), generator=g) if enc else None
    mul, res_mul = 1.0 / f, 1.0 / (f * math.sqrt(2.0))
    out, res = _pack(torch, lib, x, f, Cpad, halo, fm, ld_film if film else 0, en, Cc if enc else 0, slope, mul, True, res_mul)
    mul32, res32 = float(np.float32(mul)), float(np.float32(res_mul))  # the scalars travel as float
    xu = torch.repeat_interleave(x.double(), f, dim=1)
    v = xu
    if film:
        f3 = fm.double().view(B, T, ld_film)
        shift, scale = f3[..., :Cc], f3[..., Cc:2 * Cc]  # shift is the FIRST half
        v = (scale * v + shift) * (1.0 / math.sqrt(2.0))
    v = torch.where(v >= 0, v, float(np.float32(slope)) * v)
    if enc:
        v = v + en.double()[:, None, :]
    v = v * mul32
    real = out[:, halo:halo + T, :Cc].double()
    ulp = 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -10))) - 7)
    ratio = ((real - v).abs() / ulp).max()
    assert float(ratio) <= 1.0, float(ratio)
    assert not out[:, :halo].any() and not out[:, halo + T:].any() and not out[:, :, Cc:].any()  # exact zeros, no NaN left
    want_res = xu * res32
    r = ((res.double() - want_res).abs() / (2 * U * want_res.abs()).clamp_min(1e-300)).max()
    assert float(r) <= 1.0, float(r)


def test_pack_is_the_identity_on_bf16_values_and_the_side_output_can_stand_alone(torch, lib):
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 7, 64), generator=g).to(torch.bfloat16).float()
    out, _ = _pack(torch, lib, x, 1, 64, 8, None, 0, None, 0, 1.0, 1.0, False, 0.0)
    assert bool((out[:, 8:15].float() == x).all())
    none, res = _pack(torch, lib, x, 3, 64, 8, None, 0, None, 0, 1.0, 1.0, True, 0.5, want_out=False)
    assert none is None and bool((res == torch.repeat_interleave(x, 3, dim=1) * 0.5).all())
    # one encoding row broadcast over the batch (ld_enc = 0), as the loop passes it
    enc = torch.randn((1, 64), generator=g).to(torch.bfloat16).float() * 0.0 + 2.0
    out, _ = _pack(torch, lib, x, 1, 64, 0, None, 0, enc, 0, 1.0, 1.0, False, 0.0)
    assert bool((out.float() == (x + 2.0).to(torch.bfloat16).float()).all())


# ---- last conv + update -------------------------------------------------------------------------------------------------------------------
def _last(torch, lib, x, w, b, audio, noise, c1, c2, sigma, want_pred=True):
    B, T, Cc = x.shape
    k = w.shape[1]
    xd, wd, bd, ad = x.cuda(), w.t().contiguous().cuda(), b.cuda(), audio.cuda()
    nd = noise.cuda() if noise is not None else None
    out = torch.full((B * T + 1,), float("nan"), device="cuda")
    pred = torch.full((B * T + 1,), float("nan"), device="cuda") if want_pred else None
    _ok(lib.ma_wavegrad_last_conv_update_f32(xd.data_ptr(), B, T, Cc, wd.data_ptr(), bd.data_ptr(), k, ad.data_ptr(), _ptr(nd), c1, c2, sigma,
                                             out.data_ptr(), _ptr(pred), None))
    torch.cuda.synchronize()
    assert math.isnan(float(out[-1])) and (pred is None or math.isnan(float(pred[-1])))
    return out[:-1].cpu().view(B, T), (pred[:-1].cpu().view(B, T) if want_pred else None)


@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("B,T,Cc", [(2, 24, 64), (1, 7, 128)])
def test_last_conv_update(torch, lib, B, T, Cc, with_noise):
    g = torch.Generator().manual_seed(T * 10 + Cc)
    x, w, b = torch.randn((B, T, Cc), generator=g), torch.randn((Cc, 3), generator=g) / math.sqrt(3 * Cc), torch.randn((1,), generator=g)
    audio, noise = torch.randn((B, T), generator=g), (torch.randn((B, T), generator=g) if with_noise else None)
    c1, c2, sigma = (float(np.float32(v)) for v in (1.0954451, 0.3162278, 0.2738613))
    out, pred = _last(torch, lib, x, w, b, audio, noise, c1, c2, sigma)
    F = torch.nn.functional
    xt = x.double().transpose(1, 2)
    want_p = F.conv1d(xt, w.double()[None], b.double(), padding=1)[:, 0]
    bound_p = (3 * Cc + 4) * U * F.conv1d(xt.abs(), w.double().abs()[None], b.double().abs(), padding=1)[:, 0]
    rp = ((pred.double() - want_p).abs() / bound_p).max()
    assert float(rp) <= 1.0, float(rp)
    a = audio.double()
    want = c1 * (a - c2 * want_p)
    bound = abs(c1) * (2 * U * a.abs() + abs(c2) * (bound_p + 2 * U * want_p.abs()))
    if with_noise:
        want = want + sigma * noise.double()
        bound = bound + 2 * U * (sigma * noise.double()).abs()
    bound = bound + U * want.abs()
    ra = ((out.double() - want).abs() / bound).max()
    assert float(ra) <= 1.0, float(ra)


def test_last_conv_never_reads_the_neighbouring_utterance(torch, lib):
    T, Cc = 24, 64
    g = torch.Generator().manual_seed(5)
    x = torch.zeros((3, T, Cc))
    x[0, -1], x[2, 0] = 1000.0, -1000.0
    w, b = torch.randn((Cc, 3), generator=g), torch.randn((1,), generator=g)
    audio = torch.zeros((3, T))
    out, pred = _last(torch, lib, x, w, b, audio, None, 1.0, 1.0, 0.0)
    assert bool((pred[1] == b).all()) and float(pred[0, -1]) != float(b) and float(pred[2, 0]) != float(b)
    assert bool((out[1] == -b).all())


# ---- model ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(torch):
    """Per geometry: the weights, the inputs and, per noise level, the float64 restatement and S - computed once, never changed."""
    out = {}
    for name, (hps, shape) in GEOMETRIES.items():
        state = C.make_state(hps, 1)
        audio, spec = C.inputs(hps, shape, 11)
        refs = {}
        for level in LEVELS:
            lv = torch.tensor([level])
            ref = C.network(state, hps, audio, lv, spec)
            refs[level] = (ref, C.relrms(C.network(state, hps, audio, lv, spec, bf16_operands=True), ref))
        out[name] = dict(hps=hps, state=state, audio=audio, spec=spec, refs=refs)
    return out


@pytest.fixture(scope="module")
def models(torch, lib, cases):
    from mindaudio_amd.models import WaveGrad

    out = {}
    for name, c in cases.items():
        m = WaveGrad(c["hps"])
        m.load_state_dict(c["state"])
        out[name] = m.cuda().eval()
    return out


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_model_against_the_restatement(torch, cases, models, name, level):
    c, m = cases[name], models[name]
    ref, S = c["refs"][level]
    assert 5e-4 <= S <= 3e-2, S  # the yardstick is neither vacuous nor slack
    a, s, lv = c["audio"].cuda(), c["spec"].cuda(), torch.tensor([level], device="cuda")
    got = m(a, lv, s)
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_cuda
    err = C.relrms(got.cpu(), ref)
    print("wavegrad %s level %g: S %.3e device %.3e ratio %.2f" % (name, level, S, err, err / S))
    assert err <= 2 * S, (err, S, err / S)
    assert torch.equal(m(a, lv, s), got)  # the same bits from run to run


def test_model_levels_differ_and_a_level_per_utterance_is_its_own_row(torch, cases, models):
    c, m = cases["small"], models["small"]
    a, s = c["audio"].cuda(), c["spec"].cuda()
    lo, hi = (m(a, torch.tensor([lv], device="cuda"), s) for lv in LEVELS)
    assert not torch.equal(lo, hi) and C.relrms(lo.cpu(), hi.cpu()) > 1e-3
    both = m(a, torch.tensor(LEVELS, device="cuda"), s)  # noise_scale (B,)
    assert torch.equal(both[0], lo[0]) and torch.equal(both[1], hi[1])


def test_model_utterance_alone_agrees_with_itself_in_the_batch(torch, cases, models):
    c, m = cases["small"], models["small"]
    ref, S = c["refs"][LEVELS[0]]
    lv = torch.tensor([LEVELS[0]], device="cuda")
    batch = m(c["audio"].cuda(), lv, c["spec"].cuda())
    for b in range(c["audio"].shape[0]):
        alone = m(c["audio"][b:b + 1].cuda(), lv, c["spec"][b:b + 1].cuda())
        err = C.relrms(alone[0].cpu(), batch[b].cpu())
        assert err <= 2 * S, (b, err, S)


def test_model_uses_weights_loaded_after_a_forward(torch, cases):
    from mindaudio_amd.models import WaveGrad

    c = cases["small"]
    a, s, lv = c["audio"].cuda(), c["spec"].cuda(), torch.tensor([LEVELS[1]], device="cuda")
    m = WaveGrad(c["hps"])
    m.load_state_dict(c["state"])
    m = m.cuda().eval()
    first = m(a, lv, s)
    state2 = C.make_state(c["hps"], 2)
    m.load_state_dict(state2)
    second = m(a, lv, s)
    ref2 = C.network(state2, c["hps"], c["audio"], lv.cpu(), c["spec"])
    S2 = C.relrms(C.network(state2, c["hps"], c["audio"], lv.cpu(), c["spec"], bf16_operands=True), ref2)
    assert not torch.equal(first, second)
    assert C.relrms(second.cpu(), ref2) <= 2 * S2 and C.relrms(first.cpu(), c["refs"][LEVELS[1]][0]) <= 2 * c["refs"][LEVELS[1]][1]


# ---- reverse loop ---------------------------------------------------------------------------------------------------------------------------
BETA6 = np.linspace(1e-4, 0.3, 6)


def test_reverse_loop_against_the_restatement(torch, cases, models):
    from mindaudio_amd.wavegrad.reverse import reverse

    c, m = cases["small"], models["small"]
    hps, state, spec = c["hps"], c["state"], c["spec"]
    level = C.schedule(BETA6)[0]
    shape = (spec.shape[0], hps["hop_samples"] * spec.shape[2])
    loops = []
    for q in (False, True):
        def net(audio, n, q=q):
            return C.network(state, hps, audio, torch.tensor([float(level[n])]), spec, bf16_operands=q)

        loops.append(C.reverse_loop(net, shape, BETA6, np.random.RandomState(5)))
    S_loop = C.relrms(loops[1][0], loops[0][0])
    assert 1e-4 <= S_loop <= 3e-2, S_loop
    got, saved = reverse(m, spec, beta=BETA6, noise="numpy", seed=5, chunk=50)
    assert got.shape == shape and got.dtype == torch.float32 and got.is_cuda
    err = C.relrms(got.cpu(), loops[0][0])
    print("wavegrad loop: S_loop %.3e device %.3e ratio %.2f" % (S_loop, err, err / S_loop))
    assert err <= 2 * S_loop, (err, S_loop)
    assert sorted(saved) == sorted(loops[0][1]) == [5]  # the script's steps: (m + 1) > S - 50 and (m + 1) % 5 == 0
    assert C.relrms(saved[5].cpu(), loops[0][1][5]) <= 2 * S_loop
    got2, saved2 = reverse(m, spec, beta=BETA6, noise="numpy", seed=5, chunk=2)
    assert torch.equal(got, got2) and torch.equal(saved[5], saved2[5])  # the chunking changes no bit


def test_reverse_loop_device_noise(torch, cases, models):
    from mindaudio_amd.wavegrad.reverse import reverse

    spec = cases["small"]["spec"]
    a, _ = reverse(models["small"], spec, beta=BETA6, noise="device", seed=1)
    b, _ = reverse(models["small"], spec, beta=BETA6, noise="device", seed=2)
    a2, _ = reverse(models["small"], spec, beta=BETA6, noise="device", seed=1, chunk=3)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and not torch.equal(a, b)
    assert a.shape == (2, 240) and float(a.std()) > 0.1
    assert bool(torch.isfinite(a2).all())


def test_reverse_schedule_and_draw_order_with_a_stand_in_network(torch, cases, models):
    """The network is replaced by a known pred = 0.5 audio + 0.25; every step of the device loop is then compared with the float64
    formulas of reverse.py:116-123 applied to the device's own previous audio and the reference's np.random draws: 4 u relative."""
    from mindaudio_amd.wavegrad.reverse import reverse

    spec = cases["small"]["spec"]
    B, T = 2, 240
    beta = np.linspace(1e-3, 0.2, 7)
    level, c1, c2, sigma = C.schedule(beta)
    S = len(beta)
    trace = []

    def stand_in(audio, n):
        pred = audio * 0.5 + 0.25
        trace.append((n, audio.clone(), pred.clone()))
        return pred

    final, _ = reverse(models["small"], spec, beta=beta, noise="numpy", seed=21, chunk=3, _network=stand_in)
    assert [t[0] for t in trace] == list(range(S - 1, -1, -1))
    rng = np.random.RandomState(21)
    first = rng.normal(0, 1, [B, T]).astype(np.float32)
    assert np.array_equal(trace[0][1].cpu().numpy(), first)  # the initial audio is the first draw
    worst = 0.0
    for i, (n, audio, pred) in enumerate(trace):
        a, p = audio.cpu().double().numpy(), pred.cpu().double().numpy()
        want = c1[n] * (a - c2[n] * p)
        mag = abs(c1[n]) * (np.abs(a) + abs(c2[n]) * np.abs(p))
        if n > 0:
            z = rng.normal(0, 1, [B, T]).astype(np.float32).astype(np.float64)  # one float64 draw per step with n > 0, in order
            want, mag = want + sigma[n] * z, mag + np.abs(sigma[n] * z)
        nxt = (trace[i + 1][1] if i + 1 < S else final).cpu().double().numpy()
        worst = max(worst, float((np.abs(nxt - want) / (4 * U * mag)).max()))
    assert worst <= 1.0, worst


# ---- front end ------------------------------------------------------------------------------------------------------------------------------
def test_mel_features_against_float64_stft(torch, lib):
    from mindaudio_amd import _host
    from mindaudio_amd.wavegrad import _normalize, mel_features
    from mindaudio_amd.wavegrad.preprocess import mel_spectrum

    hps = C.YAML
    g = torch.Generator().manual_seed(17)
    t = torch.arange(6000, dtype=torch.float64)
    wav = (0.01 * torch.randn((6000,), generator=g, dtype=torch.float64) + 0.02 * torch.sin(2 * math.pi * 440.0 / 22050 * t)).float()
    got_mel = mel_spectrum(wav.numpy(), hps).cpu().double()
    got = mel_features(wav.numpy(), hps)
    win = torch.hann_window(1200, periodic=True, dtype=torch.float64)
    spec = torch.stft(wav.double(), n_fft=2048, hop_length=300, win_length=1200, window=win, center=True, pad_mode="reflect",
                      return_complex=True).abs()
    bank = torch.from_numpy(_host.mel_fbanks_f64(1025, 20.0, 22050 / 2.0, 128, 22050))
    want_mel = bank.t() @ spec
    assert got_mel.shape == want_mel.shape == (128, 21) and got.shape == (128, 21) and got.dtype == np.float32
    ratio = ((got_mel - want_mel).abs().amax(0) / (1e-5 * want_mel.abs().amax(0))).max()  # norm-wise per frame, before the logarithm
    assert float(ratio) <= 1.0, float(ratio)
    want = _normalize(want_mel.numpy()).astype(np.float64)
    inside = (want >= 1e-3) & (want < 1.0)
    assert inside.mean() > 0.9  # the signal sits between the clips
    d = np.abs(got.astype(np.float64) - want)[want >= 1e-3]
    assert float(d.max()) <= 1e-6, float(d.max())


# ---- script ---------------------------------------------------------------------------------------------------------------------------------
def test_script_writes_the_ten_files(torch, lib, cases, tmp_path, capsys):
    import mindaudio_amd.wavegrad.reverse as rv
    from mindaudio_amd.data.io import read
    from mindaudio_amd.models import WaveGrad
    from mindaudio_amd.utils import ckpt
    from mindaudio_amd.wavegrad import load_config

    c = cases["small"]
    cfg = tmp_path / "small.yaml"
    cfg.write_text(C.YAML_TEXT)
    src = WaveGrad(c["hps"])
    src.load_state_dict(c["state"])
    path = str(tmp_path / "wavegrad.ckpt")
    ckpt.write_mindspore_ckpt(path, {**ckpt.wavegrad_to_reference_names(src.state_dict()), "cur_step": np.array(4321, np.int32)})
    mel = c["spec"][0].numpy().T.copy()  # (frames, n_mels): the script transposes it
    np.save(str(tmp_path / "utt7.npy"), mel)
    save = str(tmp_path / "out")
    audio, saved = rv.main(["--config", str(cfg), "--restore", path, "--mel", str(tmp_path / "utt7.npy"), "--save", save, "--seed", "3"])
    lines = capsys.readouterr().out.splitlines()
    assert lines[:4] == ["old: utt7", "feature: (1, 64, 20)", "restore: 4321", "audio: (1, 240)"]
    steps = list(range(15, 61, 5))
    assert sorted(os.listdir(save)) == sorted("4321_predicted_utt7_%d.wav" % s for s in steps) and sorted(saved) == steps
    m = WaveGrad(load_config(str(cfg)))
    ckpt.load_mindspore_checkpoint(m, path)
    again, _ = rv.reverse(m.cuda().eval(), c["spec"][:1], seed=3, hps=load_config(str(cfg)))
    assert torch.equal(again, audio)
    wav, rate = read(os.path.join(save, "4321_predicted_utt7_60.wav"))
    assert rate == 22050 and wav.shape == (240,)
    want = np.clip(again[0].cpu().double().numpy(), -1.0, 32767.0 / 32768.0)
    assert float(np.abs(wav - want).max()) <= 1.0 / 32768.0
