"""GPU: FastSpeech2 inference (csrc/fastspeech2.hip, models/fastspeech2.py, fastspeech2/generate.py).

Kernels, each against float64 of the same inputs, with bounds that follow from the arithmetic (u = 2^-24; bf16 has 8
significant bits, unit roundoff r = 2^-8):
  attention     w_j = softmax weights, A_d = sum_j w_j |v_jd| (float64).  The device rounds every unnormalised probability to bf16 and
                sums the rounded values, so numerator and denominator carry the same relative perturbations eps_j, |eps_j| <= eps:
                |o' - o| <= 2 eps sum_j w_j |v_jd - o_d| / (1 - eps) <= 4 eps A_d / (1 - eps) ... taken as 4.1 eps A_d, with
                eps = r + 2 e_s + 64 u: e_s = (d_k + 2) u scale max_j sum_d |q_d| |k_jd| bounds the float32 score (it enters through exp as
                a relative error, twice: the score and the running max), 64 u covers __expf and one rescale per key tile.  The second
                product adds (T + 2) u A_d and the bf16 store r |o|.  With q = 0 every probability is exactly 1: eps = 0 and the
                result is the float32 mean of the valid V rows within (len + 2) u A_d + r |o|.  Masked K / V rows filled with 1e30:
                bit for bit the result with zeros there.  An utterance of length 0: exact zeros.  Guard rows behind ctx stay NaN.
  GroupNorm     moments in float64, so |y - y64| <= 3 u (|z| |gamma| + |beta|) + 1e-30 with z the normalised value, also for an input
                of 1e4 + a unit signal (a one-pass float32 variance loses all of it).  The bf16 image is the rounding of the float32
                output, bit for bit; halo rows, pad columns and masked rows exactly zero after a call on a NaN-filled buffer.
  length reg.   integers: exact equality with np.repeat; the rounding rule at half-integers and negative pre-clip values.
  variance head float32 LayerNorm of F values (ne = F / 64 per lane, then a 6-level butterfly): the mean carries (ne + 6) u mean|v|, each
                centred value u |d| more, the variance 2 (ne + 8) u relative, so the normalised z within (2 ne + 24) u (|z| + m / s),
                m = mean |v|, s = the row's standard deviation; the affine and the dot add (ne + 9) u sum |z g + b| |w|.  Taken
                together: |pred - pred64| <= (3 ne + 40) u |control| (sum_c (|z_c| + m / s) |g_c| |w_c| + sum_c |b_c| |w_c| + |bias|).
                index == searchsorted(bins, the device's own prediction, left) exactly; x_out - x is the table row bit for bit.
Model (the project's S method): S = relrms(bf16 restatement, float64 restatement) of tests/fastspeech2_cases.py, computed here on the
CPU; the device must be within 2 S of the float64 restatement (independent rounding at the same points gives sqrt(2) S, the rest
covers accumulation order).  log_duration_predictions are compared as they are; durations and indices must equal the restatement's
outside a guard band, at most 10 % of the positions guarded.  S is a relative rms over the whole tensor, so the absolute error it
stands for is S rms(v): the guard is 4 S max(|v|, rms(v)) (or 8 float32 ulps) around a bin edge - an element-wise 4 S |v| alone is
void at the zero crossings of a prediction, where the log-spaced pitch edges from 1e-5 up are densest and the bf16 restatement
itself disagrees with the float64 one - and 4 S rms(logd) exp(logd) around a half-integer of exp(logd) - 1 (the error of logd carried
through the exponential).  Durations and indices must also be exactly what the rounding rule / searchsorted give for the device's own
predictions; the continuous outputs are compared with the device's decisions injected into the restatement.  Windows: 8e-5 <= S_logd <= 2e-3,
7e-4 <= S <= 1.8e-2 for pitch, energy and mel.  The yaml cases run with p_control = 3e4 and e_control = 20: an untrained model predicts
N(0, 0.16^2), and with 255 log-spaced pitch edges 7 % apart a guard of 4 S would cover a quarter of the frames at p_control = 1; at 3e4
the predictions fall below the first edge, beyond the last one and, for a few per cent of the frames, between them.

Measured S on a CPU (weights make_state(hps, 1), inputs make_inputs(hps, lens, 2)):
  small          S_logd 3.05e-4  pitch 4.50e-3  energy 3.14e-3  mel 2.21e-3
  small, layer   S_logd 2.41e-4  pitch 3.11e-3  energy 5.41e-3  mel 2.01e-3
  yaml, 1 layer  S_logd 6.49e-4  pitch 4.27e-3  energy 5.32e-3  mel 2.29e-3
  yaml, 4 layers S_logd 3.29e-4  pitch 4.30e-3  energy 5.81e-3  mel 2.73e-3
Device against the float64 restatement on an MI355X, 2026-10-20 (S as recomputed there with the device's decisions injected):
  small          logd 3.05e-4 (S 3.05e-4)  pitch 4.51e-3 (4.50e-3)  energy 3.56e-3 (3.48e-3)  mel 2.22e-3 (2.21e-3)
  small, layer   logd 2.41e-4 (S 2.41e-4)  pitch 3.19e-3 (3.11e-3)  energy 5.45e-3 (5.41e-3)  mel 2.03e-3 (2.01e-3)
  yaml, 1 layer  logd 6.64e-4 (S 6.49e-4)  pitch 4.28e-3 (4.27e-3)  energy 5.01e-3 (5.07e-3)  mel 2.27e-3 (2.28e-3)
  yaml, 4 layers logd 4.04e-4 (S 3.29e-4)  pitch 4.71e-3 (4.30e-3)  energy 5.31e-3 (4.81e-3)  mel 2.73e-3 (2.70e-3)
Guarded positions: durations 0 .. 4.5 %, pitch indices 3.7 .. 7.8 %, energy indices 0 .. 0.9 %.  Kernels, worst error / bound: attention
0.12 .. 0.18 (d_k 128, 64, 32), variance head 0.01."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fastspeech2_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
R = 2.0 ** -8


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


# ---- attention ------------------------------------------------------------------------------------------------------------------------------
MHA_CASES = [(3, 1, 2, 128), (3, 63, 2, 128), (2, 64, 2, 128), (3, 65, 2, 128), (2, 130, 2, 128), (2, 257, 1, 128), (3, 65, 2, 64),
             (3, 65, 2, 32)]


def _lens(B, T):
    return [T, 1, 0][:B] if B == 3 else [T, max(1, T // 2 - 1)]


def _mha(torch, lib, q, k, v, lens, H, dk):
    """q, k, v (B, T, H * dk) bf16 CPU tensors, stored as three column ranges of one (B * T, 3 H dk) matrix."""
    B, T, C = q.shape
    qkv = torch.cat([q, k, v], -1).reshape(B * T, 3 * C).contiguous().cuda()
    ctx = torch.full((B * T + 2, C), float("nan"), dtype=torch.bfloat16, device="cuda")  # two guard rows behind the output
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    base = qkv.data_ptr()
    _ok(lib.ma_mha_d128_bf16(base, 3 * C, base + 2 * C, 3 * C, base + 4 * C, 3 * C, ln.data_ptr(), B, T, T, H, dk, 1.0 / math.sqrt(dk),
                             ctx.data_ptr(), C, T, None))
    torch.cuda.synchronize()
    assert bool(torch.isnan(ctx[-2:].float()).all()), "the guard rows were written"
    return ctx[:-2].cpu().view(B, T, C)


def _mha_inputs(torch, B, T, H, dk, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((B, T, H * dk), generator=g).to(torch.bfloat16) for _ in range(3))


@pytest.mark.parametrize("B,T,H,dk", MHA_CASES)
def test_attention_against_float64(torch, lib, B, T, H, dk):
    q, k, v = _mha_inputs(torch, B, T, H, dk, 100 * T + dk)
    lens = _lens(B, T)
    got = _mha(torch, lib, q, k, v, lens, H, dk).double().view(B, T, H, dk)
    scale = 1.0 / math.sqrt(dk)
    worst = 0.0
    for b, n in enumerate(lens):
        if n == 0:
            assert bool((got[b] == 0).all()), "an utterance without a valid key must be exact zeros"
            continue
        qd, kd, vd = (t[b].double().view(T, H, dk).transpose(0, 1) for t in (q, k, v))  # (H, T, dk)
        s = (qd @ kd[:, :n].transpose(1, 2)) * scale
        w = torch.softmax(s, -1)
        want = (w @ vd[:, :n]).transpose(0, 1)  # (T, H, dk)
        A = (w @ vd[:, :n].abs()).transpose(0, 1)
        e_s = (dk + 2) * U * scale * (qd.abs() @ kd[:, :n].abs().transpose(1, 2)).max(-1).values.transpose(0, 1)[..., None]  # (T, H, 1)
        eps = R + 2 * e_s + 64 * U
        bound = 4.1 * eps * A + (T + 2) * U * A + R * want.abs() + 1e-30
        worst = max(worst, float(((got[b] - want).abs() / bound).max()))
    print("attention (%d, %d, %d, %d): worst error / bound %.3f" % (B, T, H, dk, worst))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("B,T,H,dk", MHA_CASES[:6])
def test_attention_zero_query_is_the_mean_and_masked_rows_never_leak(torch, lib, B, T, H, dk):
    q, k, v = _mha_inputs(torch, B, T, H, dk, 7 * T + 1)
    lens = _lens(B, T)
    got = _mha(torch, lib, torch.zeros_like(q), k, v, lens, H, dk).double()
    for b, n in enumerate(lens):
        if n == 0:
            assert bool((got[b] == 0).all())
            continue
        mean = v[b, :n].double().mean(0)
        A = v[b, :n].double().abs().mean(0)
        bound = (n + 2) * U * A + R * mean.abs() + 1e-30
        assert bool(((got[b] - mean[None, :]).abs() <= bound[None, :]).all()), float(((got[b] - mean[None, :]).abs() / bound[None, :]).max())
    # masked rows of K and V: zeros against 1e30, bit for bit
    k0, v0, k1, v1 = k.clone(), v.clone(), k.clone(), v.clone()
    for b, n in enumerate(lens):
        k0[b, n:], v0[b, n:], k1[b, n:], v1[b, n:] = 0.0, 0.0, 1e30, 1e30
    a = _mha(torch, lib, q, k0, v0, lens, H, dk)
    c = _mha(torch, lib, q, k1, v1, lens, H, dk)
    assert bool((a.view(torch.int16) == c.view(torch.int16)).all()), "a masked key reached the result"
    assert bool(torch.isfinite(c.float()).all())


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------------
def _groupnorm(torch, lib, x, G, gamma, beta, lens, halo=4, Cpad=None):
    B, T, C = x.shape
    Cpad = Cpad or (C + 63) // 64 * 64
    parts = lib.ma_groupnorm_parts(T)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    part = torch.full((B * parts * G * 2 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((B * T + 1, C), float("nan"), device="cuda")
    img = torch.full((B * (T + 2 * halo) + 1, Cpad), float("nan"), dtype=torch.bfloat16, device="cuda")
    ln = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens is not None else None
    _ok(lib.ma_groupnorm_stats(xd.data_ptr(), B, T, C, G, part.data_ptr(), None))
    _ok(lib.ma_groupnorm_apply(xd.data_ptr(), B, T, C, Cpad, G, halo, part.data_ptr(), 1e-5, gd.data_ptr(), bd.data_ptr(), _ptr(ln),
                               out.data_ptr(), img.data_ptr(), None))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[-1]).all()) and bool(torch.isnan(img[-1].float()).all()) and bool(torch.isnan(part[-2:]).all())
    return out[:-1].cpu().view(B, T, C), img[:-1].cpu().view(B, T + 2 * halo, Cpad)


@pytest.mark.parametrize("B,T,C,G", [(2, 1, 64, 8), (3, 7, 256, 8), (2, 300, 256, 8)])
@pytest.mark.parametrize("offset", [0.0, 1e4])
def test_groupnorm(torch, lib, B, T, C, G, offset):
    g = torch.Generator().manual_seed(T + C)
    x = (torch.randn((B, T, C), generator=g) + offset).to(torch.float32)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    lens = [T, max(T - 3, 0), 1][:B]
    halo = 4
    out, img = _groupnorm(torch, lib, x, G, gamma, beta, lens, halo, Cpad=C + 64)
    xd = x.double().view(B, T, G, C // G)
    mean = xd.mean((1, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean((1, 3), keepdim=True)
    z = ((xd - mean) / torch.sqrt(var + 1e-5)).view(B, T, C)
    want = z * gamma.double() + beta.double()
    bound = 3 * U * (z.abs() * gamma.double().abs() + beta.double().abs()) + 1e-30
    for b, n in enumerate(lens):
        ratio = ((out[b, :n].double() - want[b, :n]).abs() / bound[b, :n]).max() if n else 0.0
        assert float(ratio) <= 1.0, float(ratio)
        assert bool((out[b, n:] == 0).all()), "masked rows must be exact zeros"
    assert bool((img[:, :halo] == 0).all()) and bool((img[:, halo + T:] == 0).all()) and bool((img[:, :, C:] == 0).all())
    assert bool((img[:, halo:halo + T, :C].view(torch.int16) == out.to(torch.bfloat16).view(torch.int16)).all())
    out2, img2 = _groupnorm(torch, lib, x, G, gamma, beta, lens, halo, Cpad=C + 64)
    assert bool((out.view(torch.int32) == out2.view(torch.int32)).all()) and bool((img.view(torch.int16) == img2.view(torch.int16)).all())


# ---- durations and the length regulator -----------------------------------------------------------------------------------------------------
def _regulate(torch, lib, dur, ids, cap):
    B, Ts = dur.shape
    dd, idd = torch.tensor(dur, dtype=torch.float32, device="cuda"), torch.tensor(ids, dtype=torch.int32, device="cuda")
    prefix = torch.full((B, Ts), -7, dtype=torch.int32, device="cuda")
    mel_len = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    exp = torch.full((B * cap + 1,), -7, dtype=torch.int32, device="cuda")
    _ok(lib.ma_length_regulate_i32(dd.data_ptr(), idd.data_ptr(), B, Ts, prefix.data_ptr(), mel_len.data_ptr(), exp.data_ptr(), cap, None))
    torch.cuda.synchronize()
    assert int(mel_len[-1]) == -7 and int(exp[-1]) == -7
    return prefix.cpu().numpy(), mel_len[:-1].cpu().numpy(), exp[:-1].cpu().numpy().reshape(B, cap)


def test_length_regulator_equals_repeat(torch, lib):
    rng = np.random.default_rng(0)
    Ts, cap = 300, 1001  # more phonemes than threads: every thread scans two
    dur = rng.integers(0, 5, size=(4, Ts)).astype(np.float32)
    dur[1] = 0.0                      # a row of all zeros
    dur[2] = 0.0
    dur[2, 17] = cap                  # a single phoneme of duration T_max
    dur[3, ::2] = 0.0
    ids = rng.integers(1, 300, size=(4, Ts))
    prefix, mel_len, exp = _regulate(torch, lib, dur, ids, cap)
    for b in range(4):
        want = np.repeat(ids[b], dur[b].astype(np.int32))
        assert mel_len[b] == len(want)
        assert np.array_equal(prefix[b], np.concatenate([[0], np.cumsum(dur[b].astype(np.int64))[:-1]]))
        n = min(len(want), cap)
        assert np.array_equal(exp[b, :n], want[:n]) and np.all(exp[b, n:] == 0)
    _, mel_len, exp = _regulate(torch, lib, np.array([[3.0]], np.float32), np.array([[9]]), 5)
    assert mel_len.tolist() == [3] and exp.tolist() == [[9, 9, 9, 0, 0]]


def _log_of(target):
    """A float32 logd whose correctly rounded float32 exp is exactly `target`, or None (searched over 9 neighbours of log(target))."""
    t = np.float32(target)
    lo = hi = np.float32(np.log(np.float64(t)))
    cands = [lo]
    for _ in range(4):
        lo, hi = np.nextafter(lo, np.float32(-9)), np.nextafter(hi, np.float32(9))
        cands += [lo, hi]
    hits = [c for c in cands if np.float32(np.exp(np.float64(c))) == t]
    return hits[0] if hits else None


def test_duration_rounding_rule(torch, lib):
    """Half-integers of exp(logd) - 1 that float32 can reach: 0.5 -> 0, 1.5 -> 2, 3.5 -> 4 (no float32 logd has exp(logd) = 3.5 exactly,
    so 2.5 -> 2 cannot be presented to the kernel; the rule is the same instruction).  Negative pre-clip values give 0."""
    half = {0.5: 0.0, 1.5: 2.0, 3.5: 4.0}
    logs = {v: _log_of(1.0 + v) for v in half}
    assert all(l is not None for l in logs.values()), logs
    assert _log_of(3.5) is None
    extra = np.array([-3.0, -0.1, 0.0, math.log(1.49), math.log(1.51), math.log(8.0), 0.7, 1.3], np.float32)
    logd = np.concatenate([np.array([logs[v] for v in half], np.float32), extra])
    ld = torch.tensor(logd, device="cuda")
    for ctrl in (1.0, 1.5, -1.0):
        out = torch.full((len(logd) + 1,), float("nan"), device="cuda")
        _ok(lib.ma_fs2_durations_f32(ld.data_ptr(), len(logd), ctrl, out.data_ptr(), None))
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[-1]))
        got = out[:-1].cpu().numpy()
        assert np.array_equal(got, fc.round_durations(logd, ctrl)), (ctrl, got)
        if ctrl == 1.0:
            assert got[:3].tolist() == [0.0, 2.0, 4.0] and got[3:6].tolist() == [0.0, 0.0, 0.0] and got[6:9].tolist() == [0.0, 1.0, 7.0]
        if ctrl == -1.0:
            assert got[3] == 1.0 and got[1] == 0.0  # round(exp(-3) - 1) = -1, times -1; -2 clips to 0


# ---- variance head ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,F,C,n_bins,halo", [(2, 5, 64, 64, 16, 4), (3, 37, 256, 256, 256, 4)])
def test_variance_head(torch, lib, B, T, F, C, n_bins, halo):
    g = torch.Generator().manual_seed(F + T)
    hid = torch.relu(torch.randn((B, T, F), generator=g))
    gamma, beta = 1 + 0.2 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    w, bias = torch.randn(F, generator=g) / math.sqrt(F), torch.tensor([0.3])
    bins = torch.linspace(-1.5, 1.5, n_bins - 1)
    table, x, pos = torch.randn((n_bins, C), generator=g), torch.randn((B, T, C), generator=g), torch.randn((T, C), generator=g)
    lens = [T, 2, 0][:B]
    control = 1.25
    dev = lambda t: t.cuda() if t is not None else None
    hd, gd, bd, wd, biasd, binsd, td, xd, pd = (dev(t) for t in (hid, gamma, beta, w, bias, bins, table, x, pos))

    def run(lens_, bins_, pos_, want_img=True, index_in=None, n_edges=None):
        pred = torch.full((B * T + 1,), float("nan"), device="cuda")
        idx = torch.full((B * T + 1,), -7, dtype=torch.int32, device="cuda")
        xo = torch.full((B * T + 1, C), float("nan"), device="cuda")
        xp = torch.full((B * T + 1, C), float("nan"), device="cuda") if pos_ is not None else None
        img = torch.full((B * (T + 2 * halo) + 1, C), float("nan"), dtype=torch.bfloat16, device="cuda") if want_img else None
        ln = torch.tensor(lens_, dtype=torch.int32, device="cuda") if lens_ is not None else None
        _ok(lib.ma_variance_head_f32(hd.data_ptr(), B, T, F, gd.data_ptr(), bd.data_ptr(), 1e-7, wd.data_ptr(), biasd.data_ptr(), _ptr(ln),
                                     control, pred.data_ptr(), _ptr(bins_), n_bins if n_edges is None else n_edges + 1, _ptr(index_in),
                                     idx.data_ptr(), td.data_ptr(),
                                     xd.data_ptr(), _ptr(pos_), C, halo, xo.data_ptr(), _ptr(xp), _ptr(img), None))
        torch.cuda.synchronize()
        assert bool(torch.isnan(pred[-1])) and int(idx[-1]) == -7 and bool(torch.isnan(xo[-1]).all())
        return (pred[:-1].cpu().view(B, T), idx[:-1].cpu().view(B, T), xo[:-1].cpu().view(B, T, C),
                xp[:-1].cpu().view(B, T, C) if xp is not None else None, img[:-1].cpu().view(B, T + 2 * halo, C) if img is not None else None)

    pred, idx, xo, xp, img = run(None, binsd, pd)
    h64 = hid.double()
    mean = h64.mean(-1, keepdim=True)
    s = torch.sqrt(((h64 - mean) ** 2).mean(-1, keepdim=True) + 1e-7)
    z = (h64 - mean) / s
    want = ((z * gamma.double() + beta.double()) @ w.double() + 0.3) * control
    ne = F // 64
    m_over_s = h64.abs().mean(-1, keepdim=True) / s
    bound = (3 * ne + 40) * U * control * (((z.abs() + m_over_s) * gamma.double().abs() * w.double().abs()).sum(-1)
                                           + (beta.double().abs() * w.double().abs()).sum() + 0.3)
    ratio = float(((pred.double() - want).abs() / bound).max())
    print("variance head F = %d: worst error / bound %.3f" % (F, ratio))
    assert ratio <= 1.0, ratio
    assert np.array_equal(idx.numpy(), np.searchsorted(bins.numpy(), pred.numpy(), "left"))
    assert idx.min() >= 0 and idx.max() <= n_bins - 1 and len(np.unique(idx.numpy())) > 2
    assert bool(((xo - x).view(torch.int32) == (x + table[idx.long()] - x).view(torch.int32)).all())
    assert bool((xo.view(torch.int32) == (x + table[idx.long()]).view(torch.int32)).all())
    assert bool((xp.view(torch.int32) == ((x + table[idx.long()]) + pos[None]).view(torch.int32)).all())
    assert bool((img[:, :halo] == 0).all()) and bool((img[:, halo + T:] == 0).all())
    assert bool((img[:, halo:halo + T].view(torch.int16) == xp.to(torch.bfloat16).view(torch.int16)).all())
    # a mask zeroes the prediction before the control; the duration form (no table) writes the prediction only
    pred_m = run(lens, binsd, None)[0]
    for b, n in enumerate(lens):
        assert bool((pred_m[b, :n] == pred[b, :n]).all()) and bool((pred_m[b, n:] == 0).all())
    # predictions exactly on an edge, just above it and beyond each end, through bins placed at the device's own predictions
    flat = np.sort(np.unique(pred.numpy().reshape(-1)))
    assert len(flat) >= 5
    edges = flat[1:-1][::max(1, (len(flat) - 2) // (n_bins - 1) + 1)]  # the device's own predictions, the smallest and largest left out
    assert 3 <= len(edges) <= n_bins - 1
    p2, i2 = run(None, torch.tensor(edges, device="cuda"), None, want_img=False, n_edges=len(edges))[:2]
    assert bool((p2 == pred).all())
    assert np.array_equal(i2.numpy(), np.searchsorted(edges, pred.numpy(), "left"))
    on_edge = np.isin(pred.numpy(), edges)
    assert on_edge.sum() >= len(edges) and (np.asarray(edges)[i2.numpy()[on_edge]] == pred.numpy()[on_edge]).all()  # side left
    assert i2.min() == 0 and i2.max() == len(edges)  # below the first edge and beyond the last
    # given indices replace the search
    forced = torch.randint(0, n_bins, (B, T), generator=g).to(torch.int32)
    i3, xo3 = run(None, binsd, None, want_img=False, index_in=forced.cuda())[1:3]
    assert bool((i3 == forced).all()) and bool((xo3.view(torch.int32) == (x + table[forced.long()]).view(torch.int32)).all())


# ---- model ----------------------------------------------------------------------------------------------------------------------------------
MODEL_CASES = {  # hps, src_lens, norm, p_control, e_control
    "small": (fc.SMALL, [1, 5, 12], "group", 1.0, 1.0),
    "small_layer": (fc.SMALL, [1, 5, 12], "layer", 1.0, 1.0),
    "yaml": (fc.YAML, [7, 11], "group", 3e4, 20.0),
    "yaml4": (fc.YAML4, [20], "group", 3e4, 20.0),
}
S_LOGD, S_CONT, CAP = (8e-5, 2e-3), (7e-4, 1.8e-2), 0.10


def _model(torch, hps, norm, state):
    from mindaudio_amd.models import FastSpeech2

    m = FastSpeech2(hps, norm=norm)
    m.load_state_dict(state)
    return m.cuda().eval()


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_against_restatement(torch, case):
    hps, src_lens, norm, pc, ec = MODEL_CASES[case]
    state = fc.make_state(hps, 1)
    texts, lens = fc.make_inputs(hps, src_lens, seed=2)
    kw = dict(p_control=pc, e_control=ec, d_control=1.0, norm=norm)
    ref = fc.infer(hps, state, texts, lens, **kw)
    rbf = fc.infer(hps, state, texts, lens, bf16_operands=True, **kw)
    model = _model(torch, hps, norm, state)
    out = model.infer(None, texts, lens, texts.shape[1], p_control=pc, e_control=ec, d_control=1.0)
    torch.cuda.synchronize()
    # log durations
    S = fc.relrms(rbf["log_duration_predictions"], ref["log_duration_predictions"])
    logd = _np(out["log_duration_predictions"])
    err = fc.relrms(logd, ref["log_duration_predictions"])
    print("%s: S_logd %.3e device %.3e" % (case, S, err))
    assert S_LOGD[0] <= S <= S_LOGD[1], S
    assert err <= 2 * S, (err, S)
    # durations: equal to the restatement's away from the half-integers, and exactly the rule applied to the device's own predictions
    em = ref["exp_minus_one"]
    rms = math.sqrt(float(np.mean(ref["log_duration_predictions"] ** 2)))
    guard = np.maximum(4 * S * rms * (em + 1.0), 8 * U * (em + 1.0))
    near = np.abs(em - np.floor(em) - 0.5) <= guard
    near_bf = near & (rbf["duration_rounded"] != ref["duration_rounded"])
    dur = _np(out["duration_rounded"])
    assert near.mean() <= CAP, near.mean()
    assert np.array_equal(rbf["duration_rounded"][~near], ref["duration_rounded"][~near]), int(near_bf.sum())
    assert np.array_equal(dur[~near], ref["duration_rounded"][~near])
    assert np.array_equal(dur, fc.round_durations(logd, 1.0))
    mel_len = _np(out["mel_len"])
    assert np.array_equal(mel_len, dur.astype(np.int32).sum(1)) and out["mel_predictions"].shape[1] == int(mel_len.max())
    assert np.array_equal(_np(out["src_masks"]), ref["src_masks"])
    # the continuous outputs with the device's decisions injected
    pidx, eidx = _np(out["pitch_index"]), _np(out["energy_index"])
    pbins, ebins = state["variance_adaptor.pitch_bins"].numpy(), state["variance_adaptor.energy_bins"].numpy()
    pitch, energy = _np(out["pitch_predictions"]), _np(out["energy_predictions"])
    assert np.array_equal(pidx, np.searchsorted(pbins, pitch, "left")) and np.array_equal(eidx, np.searchsorted(ebins, energy, "left"))
    ov = {"durations": dur, "pitch_index": pidx, "energy_index": eidx}
    ref2 = fc.infer(hps, state, texts, lens, overrides=ov, **kw)
    rbf2 = fc.infer(hps, state, texts, lens, bf16_operands=True, overrides=ov, **kw)
    assert np.array_equal(_np(out["mel_masks"])[:, 0], ref2["mel_masks"])
    for key in ("pitch_predictions", "energy_predictions", "mel_predictions", "output"):
        Sk = fc.relrms(rbf2[key], ref2[key])
        ek = fc.relrms(_np(out[key]), ref2[key])
        print("%s: %s S %.3e device %.3e" % (case, key, Sk, ek))
        if key != "output":  # (the adaptor's output is the encoder's plus two table rows: it has the mel's S, not a window of its own)
            assert S_CONT[0] <= Sk <= S_CONT[1], (key, Sk)
        assert ek <= 2 * Sk, (key, ek, Sk)
    # indices: equal to the restatement's (same durations injected, own indices) away from the bin edges
    free = fc.infer(hps, state, texts, lens, overrides={"durations": dur}, **kw)
    free_bf = fc.infer(hps, state, texts, lens, bf16_operands=True, overrides={"durations": dur}, **kw)
    for name, bins, key, idx in (("pitch", pbins, "pitch_predictions", pidx), ("energy", ebins, "energy_predictions", eidx)):
        if name == "energy":  # the energy predictor sees the pitch embedding: hold the pitch indices at the device's
            free = fc.infer(hps, state, texts, lens, overrides={"durations": dur, "pitch_index": pidx}, **kw)
            free_bf = fc.infer(hps, state, texts, lens, bf16_operands=True, overrides={"durations": dur, "pitch_index": pidx}, **kw)
        v = free[key]
        Sv = fc.relrms(free_bf[key], v)
        guard = np.maximum(4 * Sv * np.maximum(np.abs(v), math.sqrt(float(np.mean(v ** 2)))), 8 * U * np.abs(v))
        near = (np.abs(v[..., None] - bins.astype(np.float64)[None, None, :]) <= guard[..., None]).any(-1)
        want = np.searchsorted(bins, v.astype(np.float32), "left")
        print("%s: %s indices guarded %.3f, range %d .. %d" % (case, name, near.mean(), idx.min(), idx.max()))
        assert near.mean() <= CAP, (name, near.mean())
        assert np.array_equal(free_bf[name + "_index"][~near], want[~near])
        assert np.array_equal(idx[~near], want[~near]), name


def test_model_is_deterministic_and_batch_independent(torch):
    hps, src_lens, norm, pc, ec = MODEL_CASES["small"]
    state = fc.make_state(hps, 1)
    texts, lens = fc.make_inputs(hps, src_lens, seed=2)
    model = _model(torch, hps, norm, state)
    a = model.infer(None, texts, lens, texts.shape[1])
    b = model.infer(None, texts, lens, texts.shape[1])
    for key in ("mel_predictions", "pitch_predictions", "energy_predictions", "log_duration_predictions", "output"):
        assert bool((a[key].contiguous().view(torch.int32) == b[key].contiguous().view(torch.int32)).all()), key
    # the utterance with the longest mel alone, padded to the batch's text length: its frames are the batch's, so are its bits
    i = int(a["mel_len"].argmax())
    c = model.infer(None, texts[i:i + 1], lens[i:i + 1], texts.shape[1])
    assert c["mel_predictions"].shape[1] == a["mel_predictions"].shape[1]
    for key in ("mel_predictions", "pitch_predictions", "energy_predictions", "log_duration_predictions", "output"):
        assert bool((a[key][i:i + 1].contiguous().view(torch.int32) == c[key].contiguous().view(torch.int32)).all()), key


def test_model_refuses_what_the_reference_cannot_run(torch):
    hps = fc.SMALL
    state = fc.make_state(hps, 1, duration_bias=math.log(8.0))  # 7 frames a phoneme: 12 phonemes pass max_seq_len + 1 = 65
    texts, lens = fc.make_inputs(hps, [12], seed=2)
    model = _model(torch, hps, "group", state)
    with pytest.raises(ValueError, match="max_seq_len"):
        model.infer(None, texts, lens, 12)
    bad = texts.copy()
    bad[0, 3] = 0
    with pytest.raises(ValueError, match="PAD"):
        model.infer(None, bad, lens, 12)
    # one utterance with every duration 0 beside one that expands: zeros from the attention, no NaN anywhere
    st = fc.make_state(hps, 1)
    texts, lens = fc.make_inputs(hps, [3, 6], seed=2)
    model = _model(torch, hps, "group", st)
    dur = np.zeros((2, 6), np.float32)
    dur[1, :6] = 2.0
    out = model.infer(None, texts, lens, 6, _overrides={"durations": dur})
    assert _np(out["mel_len"]).tolist() == [0.0, 12.0] and bool(torch.isfinite(out["mel_predictions"]).all())


# ---- script ---------------------------------------------------------------------------------------------------------------------------------
def test_generate_script_writes_the_models_output(torch, tmp_path):
    from mindaudio_amd.fastspeech2 import generate
    from mindaudio_amd.utils import ckpt

    hps = fc.SMALL
    state = fc.make_state(hps, 4)
    path, ids_path = str(tmp_path / "fs2.ckpt"), str(tmp_path / "ids.npy")
    ckpt.write_mindspore_ckpt(path, ckpt.fastspeech2_to_reference_names(state))
    ids = np.array([5, 9, 2, 31, 7, 7, 12], np.int64)
    np.save(ids_path, ids)
    generate.main(["--restore", path, "--ids", ids_path, "--save", str(tmp_path)], hps=hps)
    got = np.load(str(tmp_path / "msfs2_0.npy"))
    model = _model(torch, hps, "group", state)
    want = _np(model.infer(None, ids[None], np.array([7]), 7)["mel_predictions"])
    assert got.shape == want.shape and got.shape[0] == 1 and got.shape[2] == 16
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_generate_script_hands_the_mel_to_the_vocoder(torch, tmp_path):
    import wavegrad_cases as wc
    from mindaudio_amd.data.io import read
    from mindaudio_amd.fastspeech2 import generate
    from mindaudio_amd.models import WaveGrad
    from mindaudio_amd.utils import ckpt
    from mindaudio_amd.wavegrad import load_config
    from mindaudio_amd.wavegrad.reverse import reverse

    hps = fc.H(dict(fc.SMALL, n_mels=64, hop_samples=12))  # the small vocoder's mel geometry
    fs2_path, voc_path, ids_path, cfg = (str(tmp_path / n) for n in ("fs2.ckpt", "wavegrad.ckpt", "ids.npy", "small.yaml"))
    ckpt.write_mindspore_ckpt(fs2_path, ckpt.fastspeech2_to_reference_names(fc.make_state(hps, 4)))
    ckpt.write_mindspore_ckpt(voc_path, ckpt.wavegrad_to_reference_names(wc.make_state(wc.SMALL, 1)))
    open(cfg, "w").write(wc.YAML_TEXT)
    np.save(ids_path, np.array([5, 9, 2, 31], np.int64))
    argv = ["--restore", fs2_path, "--ids", ids_path, "--save", str(tmp_path), "--vocoder", voc_path, "--config", cfg, "--seed", "3"]
    out = generate.main(argv, hps=hps)
    mel = np.load(str(tmp_path / "msfs2_0.npy"))
    frames = mel.shape[1]
    assert mel.shape == (1, frames, 64) and frames == int(out["mel_len"][0])
    vocoder = WaveGrad(load_config(cfg))
    ckpt.load_mindspore_checkpoint(vocoder, voc_path)
    want, _ = reverse(vocoder.cuda().eval(), np.ascontiguousarray(mel.transpose(0, 2, 1)), seed=3, hps=load_config(cfg))
    wav, rate = read(str(tmp_path / "msfs2_0.wav"))
    assert rate == 22050 and wav.shape == (12 * frames,)
    assert float(np.abs(wav - np.clip(want[0].cpu().double().numpy(), -1.0, 32767.0 / 32768.0)).max()) <= 1.0 / 32768.0
    with pytest.raises(ValueError, match="mel geometry"):  # a vocoder of another geometry is refused, not converted
        generate.main(["--ids", ids_path, "--save", str(tmp_path), "--vocoder", voc_path, "--config", cfg], hps=fc.SMALL)
