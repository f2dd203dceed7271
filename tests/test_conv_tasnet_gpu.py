"""GPU: Conv-TasNet separation (csrc/conv_tasnet.hip, models/conv_tasnet.py, loss/separation_loss.py, conv_tasnet/eval.py).

Entry points, each against float64 of the same float32 inputs, with bounds that follow from the arithmetic (u = 2^-24):
  encode          |d| <= (L + 2) u sum_j |x_j| |w_j| per output (L fused multiply-adds and the sum's growth); K by the floor.
  prelu + stats   outputs exact (the weights are powers of two); each partial's sum within (n + 4) 2^-53 sum |y| of the float64 sum
                  of the device's own outputs, its centred second moment within (n + 8) 2^-53 relative (n-term float64 sums).
  gln + dwconv    |d| <= 8 u sum_p |w_p| A with A = max |n| + |mean| rstd: the normalised value carries 3 u relative plus the
                  rounding of the float32 mean (|mean| u rstd), three taps add 3 u, PReLU one more.  An all-zero utterance between
                  two that end / begin with an impulse stays EXACTLY zero at every dilation (no tap crosses an utterance).
  gln apply       one bf16 ulp of max(|n|, 2^-10): round-to-nearest is half an ulp, the float32 error in front of it is far
                  below the other half except at zero crossings, which the floor covers.
  decode          |d| <= (N + 8) u x the same overlap of |relu(score) mixture_w| . |basis|; the pad samples are exactly zero.
  si_snr          within 1e-4 dB of the two-pass float64 formula (float64 accumulation leaves ~1e-9; the margin covers a float32
                  logarithm); the diagonal at full length equals the reference's cal_SISNR (tests/golden/separation_sisnr.npz).
Model: S = relrms((b), (a)) of tests/conv_tasnet_cases.py is computed here on the CPU; the device must be within 2 S of (a)
(the device rounds where (b) rounds, independently: sqrt(2) S; the rest covers float32 accumulation order), and S <= 3e-2.

Measured on an MI355X (S, device):  small 8.63e-3, 8.66e-3;  yaml 1.00e-2, 9.86e-3;  small, true overlap 8.63e-3, 8.69e-3
(DESIGN.md "Conv-TasNet")."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import conv_tasnet_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


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


def _join(part):
    """(mean, var) per utterance of (M, P, 3) partials, Chan's update in float64."""
    n, s, m2 = part[..., 0], part[..., 1], part[..., 2]
    N = n.sum(1)
    mean = s.sum(1) / N
    M2 = (m2 + n * (s / n - mean[:, None]) ** 2).sum(1)
    return mean, M2 / N


def _check_join(part, values):
    """The joined partials against the float64 moments of the values they describe ((M, n) array): the mean within
    (n + 4) 2^-53 mean |v| (an n-term float64 sum), the variance within 4 (n + 8) 2^-53 relative (the tiles' sums and Chan's join)."""
    mean, var = _join(part)
    n = values.shape[1]
    assert np.all(np.abs(mean - values.mean(1)) <= (n + 4) * 2.0 ** -53 * np.abs(values).mean(1))
    assert np.all(np.abs(var - values.var(1)) <= 4 * (n + 8) * 2.0 ** -53 * values.var(1))


def _stats(torch, lib, y, weight=1.0):
    """ma_prelu_gln_stats on y (M, K, C): (output, partials (M, P, 3) on the device)."""
    M, K, Cc = y.shape
    P = lib.ma_tasnet_stat_parts(K, Cc)
    out = torch.empty_like(y)
    part = torch.full((M, P, 3), float("nan"), dtype=torch.float64, device=y.device)
    w = torch.tensor([weight], dtype=torch.float32, device=y.device)
    _ok(lib.ma_prelu_gln_stats(y.data_ptr(), M, K, Cc, w.data_ptr(), out.data_ptr(), part.data_ptr(), None))
    return out, part


@pytest.mark.parametrize("T,L", [(330, 20), (339, 20), (136, 16)])
def test_encode(torch, lib, T, L):
    M, N = 2, 64
    g = torch.Generator().manual_seed(T + L)
    x = torch.randn((M, T), generator=g)
    w = torch.randn((N, 1, L), generator=g) * 0.3
    K = (T - L) // (L // 2) + 1
    assert K == {(330, 20): 32, (339, 20): 32, (136, 16): 16}[(T, L)]
    P = lib.ma_tasnet_stat_parts(K, N)
    xd, wt = x.cuda(), w[:, 0].t().contiguous().cuda()
    mw = torch.full((M * K + 1, N), float("nan"), device="cuda")  # one guard row behind the output
    part = torch.empty((M, P, 3), dtype=torch.float64, device="cuda")
    _ok(lib.ma_tasnet_encode_f32(xd.data_ptr(), M, T, T, wt.data_ptr(), L, N, mw.data_ptr(), part.data_ptr(), None))
    got = mw[:M * K].cpu().double().view(M, K, N)
    assert torch.isnan(mw[M * K:]).all()  # nothing written past K frames (the trailing samples of T = 339 make no frame)
    F = torch.nn.functional
    want = F.relu(F.conv1d(x.double()[:, None], w.double(), stride=L // 2)).transpose(1, 2)
    bound = (L + 2) * U * F.conv1d(x.double().abs()[:, None], w.double().abs(), stride=L // 2).transpose(1, 2)
    assert want.shape == got.shape and bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())
    _check_join(part.cpu().numpy(), got.numpy().reshape(M, -1))


@pytest.mark.parametrize("weight", [0.25, -0.5])
def test_prelu_stats(torch, lib, weight):
    g = torch.Generator().manual_seed(11)
    x = torch.randn((3, 37, 128), generator=g) + 0.3
    out, part = _stats(torch, lib, x.cuda(), weight)
    want = torch.where(x >= 0, x, weight * x)  # exact: the weight is a power of two
    assert torch.equal(out.cpu(), want)
    part = part.cpu().numpy()
    assert part.shape == (3, 1, 3)
    y = want.double().numpy().reshape(3, -1)
    n = y.shape[1]
    assert np.array_equal(part[:, 0, 0], np.full(3, float(n)))
    assert np.all(np.abs(part[:, 0, 1] - y.sum(1)) <= (n + 4) * 2.0 ** -53 * np.abs(y).sum(1))
    m2 = ((y - y.mean(1, keepdims=True)) ** 2).sum(1)
    assert np.all(np.abs(part[:, 0, 2] - m2) <= (n + 8) * 2.0 ** -53 * m2)


def _dwconv(torch, lib, y, w, dil, a2):
    """gLN -> depthwise conv -> PReLU on y (M, K, H) with w (H, 1, 3): (z on the device, its partials)."""
    M, K, H = y.shape
    _, part_in = _stats(torch, lib, y)  # weight 1: y as it is, and its moments
    P = lib.ma_tasnet_stat_parts(K, H)
    z = torch.full((M, K, H), float("nan"), device="cuda")
    part = torch.empty((M, P, 3), dtype=torch.float64, device="cuda")
    wt = w[:, 0].t().contiguous().cuda()
    a = torch.tensor([a2], dtype=torch.float32, device="cuda")
    _ok(lib.ma_gln_dwconv_prelu(y.data_ptr(), M, K, H, part_in.data_ptr(), wt.data_ptr(), 3, dil, a.data_ptr(), z.data_ptr(),
                                part.data_ptr(), None))
    return z, part, part_in


@pytest.mark.parametrize("K", [100, 129, 300])
def test_gln_dwconv_prelu(torch, lib, K):
    M, H = 3, 128
    F = torch.nn.functional
    g = torch.Generator().manual_seed(K)
    y = torch.randn((M, K, H), generator=g) * 2 + 0.5
    w = torch.randn((H, 1, 3), generator=g)
    y64 = y.double().transpose(1, 2)  # (M, H, K)
    n64 = C.gln(y64)
    mean = y64.mean(dim=(1, 2))
    rstd = 1.0 / torch.sqrt(y64.var(dim=(1, 2), unbiased=False) + C.EPS)
    A = float(n64.abs().max() + (mean.abs() * rstd).max())
    tol = (8 * U * A * w.double().abs().sum(dim=(1, 2)))[None, None, :]  # per channel
    for d in (1, 2, 64, 128):  # d = 128 > K = 100 leaves only the centre tap
        z, part, _ = _dwconv(torch, lib, y.cuda(), w, d, 0.25)
        want = F.prelu(F.conv1d(n64, w.double(), padding=d, dilation=d, groups=H), torch.tensor([0.25], dtype=torch.float64))
        got = z.cpu().double()
        err = (got - want.transpose(1, 2)).abs()
        assert bool((err <= tol).all()), (d, float((err / tol).max()))
        if d >= K:
            centre = F.prelu(n64 * w.double()[:, 0, 1][None, :, None],torch.tensor([0.25], dtype=torch.float64)).transpose(1, 2)
            assert bool(((got - centre).abs() <= tol).all())
        # the partials describe the device's own output
        _check_join(part.cpu().numpy(), got.numpy().reshape(M, -1))


@pytest.mark.parametrize("K", [100, 129, 300])
def test_dwconv_never_crosses_an_utterance(torch, lib, K):
    """Utterance 1 ends and utterance 3 begins with an impulse (so their normalised values are non-zero everywhere); utterance 2 is
    all zeros, normalises to zeros, and must come out EXACTLY zero: a tap that read a neighbour's row would show."""
    H = 128
    y = torch.zeros((3, K, H))
    y[0, K - 1] = 5.0
    y[2, 0] = -7.0
    w = torch.ones((H, 1, 3))
    for d in (1, 2, 64, 128):
        z, _, _ = _dwconv(torch, lib, y.cuda(), w, d, 0.25)
        z = z.cpu()
        assert not z[1].any(), d
        assert bool(torch.isfinite(z).all())


@pytest.mark.parametrize("K", [100, 129, 300])
def test_gln_apply_bf16(torch, lib, K):
    M, H = 3, 128
    g = torch.Generator().manual_seed(K + 1)
    y = torch.randn((M, K, H), generator=g) * 3 - 1.0
    yd = y.cuda()
    _, part = _stats(torch, lib, yd)
    out = torch.empty((M, K, H), dtype=torch.bfloat16, device="cuda")
    _ok(lib.ma_gln_apply_bf16(yd.data_ptr(), M, K, H, part.data_ptr(), out.data_ptr(), None))
    n64 = C.gln(y.double().transpose(1, 2)).transpose(1, 2)
    ulp = 2.0 ** (torch.floor(torch.log2(n64.abs().clamp_min(2.0 ** -10))) - 7)  # bf16: 8 significant bits
    err = (out.cpu().double() - n64).abs()
    assert bool((err <= ulp).all()), float((err / ulp).max())


@pytest.mark.parametrize("overlap", ["paired", "true"])
@pytest.mark.parametrize("K,L", [(32, 20), (15, 16)])
def test_decode(torch, lib, K, L, overlap):
    M, Cs, N = 2, 2, 64
    g = torch.Generator().manual_seed(K * 100 + L)
    score = torch.randn((M, K, Cs * N), generator=g)
    mw = torch.randn((M, K, N), generator=g).abs()
    basis = torch.randn((L, N), generator=g) * 0.2
    h = L // 2
    out = torch.full((M, Cs, (K + 1) * h), float("nan"), device="cuda")
    sd, md, bd = score.cuda(), mw.cuda(), basis.cuda()
    _ok(lib.ma_tasnet_decode_f32(sd.data_ptr(), md.data_ptr(), M, K, Cs, N, bd.data_ptr(), L, {"paired": 0, "true": 1}[overlap],
                                 out.data_ptr(), None))
    s = torch.relu(score.double()).view(M, K, Cs, N).transpose(1, 2) * mw.double()[:, None]  # (M, C, K, N)
    frames = s @ basis.double().t()
    mag = s.abs() @ basis.double().abs().t()
    fold = C.overlap_paired if overlap == "paired" else C.overlap_true
    want, bound = fold(frames), (N + 8) * U * fold(mag)
    got = out.cpu().double()
    assert got.shape == want.shape
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    if overlap == "paired":
        assert not got[..., K * h:].any()  # the pad is exactly zero
        assert torch.equal(want[..., :K * h], C.overlap_paired_reference(frames))  # and the body is the reference's matrix product
    else:
        assert bool((got[..., K * h:] != 0).any())


@pytest.fixture(scope="module")
def snr_inputs(torch):
    g = np.load(C.GOLDENS)
    rng = np.random.RandomState(3)

    def build(Cs):
        T = 1000
        src = rng.randn(3, Cs, T).astype(np.float32)
        est = (src + 0.5 * rng.randn(3, Cs, T)).astype(np.float32)
        gold = [5, 0, 2][:Cs]  # utterance 0: golden pairs (5: the target plus -60 dB noise)
        for c, k in enumerate(gold):
            src[0, c], est[0, c] = g["ref%d" % k], g["est%d" % k]
        src[1, 1] = 0.0  # a silent target
        return src, est, np.array([1000, 777, 1]), [float(g["sisnr"][k]) for k in gold]

    return {Cs: build(Cs) for Cs in (2, 3)}


@pytest.mark.parametrize("Cs", [2, 3])
def test_si_snr_pit(torch, snr_inputs, Cs):
    from mindaudio_amd import ops
    from mindaudio_amd.loss import Convtasnet_Loss

    src, est, lengths, gold = snr_inputs[Cs]
    want = C.si_snr_pairwise(src, est, lengths)
    assert want[1, 0, 1] == pytest.approx(-80.0, abs=1e-6)  # the silent target
    assert want[0, 0, 0] == pytest.approx(60.0, abs=1.0)    # the -60 dB pair
    for swap in (False, True):
        e = est[:, ::-1].copy() if swap else est  # estimates in reverse channel order: the permutation must undo it
        w = want[:, ::-1] if swap else want
        ed = torch.from_numpy(e).cuda()
        keep = ed.clone()
        loss, max_snr, reordered, perm, pair = ops.si_snr_pit(torch.from_numpy(src).cuda(), ed, torch.from_numpy(lengths))
        assert torch.equal(ed, keep)  # the caller's estimate is unchanged
        pair = pair.cpu().numpy()
        assert pair.dtype == np.float64 and np.abs(pair - w).max() <= 1e-4, np.abs(pair - w).max()
        if not swap:
            for c, v in enumerate(gold):  # the diagonal at full length is the reference's cal_SISNR
                assert abs(pair[0, c, c] - v) <= 1e-4, (c, pair[0, c, c], v)
        perm = perm.cpu().numpy()
        snrs = []
        for b in range(3):
            p, v = C.best_permutation(w[b])
            assert tuple(perm[b]) == p, (b, perm[b], p)
            snrs.append(v)
            r = reordered[b].cpu().numpy()
            n = lengths[b]
            assert np.array_equal(r[:, :n], e[b, list(p), :n]) and not r[:, n:].any()
        if swap:
            assert tuple(perm[0]) == tuple(range(Cs))[::-1] and np.array_equal(reordered[0].cpu().numpy(), est[0])
        assert tuple(perm[2]) == tuple(range(Cs))  # length 1: every pair is -80 dB, the first permutation wins the tie
        assert max_snr.shape == (3, 1) and np.allclose(max_snr.cpu().numpy()[:, 0], snrs, rtol=0, atol=1e-4)
        assert float(loss) == pytest.approx(-np.mean(snrs), abs=1e-4)
        l2, m2, e2, r2 = Convtasnet_Loss()(torch.from_numpy(src).cuda(), ed, torch.from_numpy(lengths).cuda())
        assert e2 is ed and torch.equal(r2, reordered) and torch.equal(m2, max_snr) and float(l2) == float(loss)


def test_si_snr_refuses_bad_lengths_and_handles_device_lengths(torch):
    from mindaudio_amd import ops

    src = torch.randn((2, 2, 50), device="cuda")
    est = src + 0.1 * torch.randn((2, 2, 50), device="cuda")
    for bad in ([50, 0], [51, 10], [50], [50.0, 10.0]):
        with pytest.raises(ValueError):
            ops.si_snr_pairwise(src, est, bad)
    # lengths on the device are not read back: the kernel clamps them, and an empty utterance is -80 dB throughout
    pair = ops.si_snr_pairwise(src, est, torch.tensor([70, 0], device="cuda")).cpu().numpy()
    want = C.si_snr_pairwise(src.cpu().numpy(), est.cpu().numpy(), [50, 50])
    assert np.abs(pair[0] - want[0]).max() <= 1e-4
    assert np.abs(pair[1] + 80.0).max() <= 1e-4


# ---- the model ----------------------------------------------------------------------------------------------------------------------
CASES = {"small": (C.SMALL, 3, 3010, 1), "yaml": (C.YAML, 1, 4010, 2)}


@pytest.fixture(scope="module")
def model_refs():
    """(state, mixture, (a), S) per case, computed once on the CPU and left unchanged."""
    out = {}
    for name, (cfg, M, T, seed) in CASES.items():
        state, x = C.make_state(cfg, seed), C.make_mixture(M, T, seed + 10)
        a = C.forward(state, cfg, x)
        S = C.relrms(C.forward(state, cfg, x, bf16_operands=True), a)
        out[name] = (state, x, a, S)
    return out


def _model(cfg, state, **kw):
    from mindaudio_amd.models import ConvTasNet

    m = ConvTasNet(**cfg, **kw)
    m.load_state_dict(state)
    return m.cuda().eval()


@pytest.mark.parametrize("name", ["small", "yaml"])
def test_model_forward(torch, model_refs, name):
    cfg, M, T, _ = CASES[name]
    state, x, a, S = model_refs[name]
    assert 1e-3 <= S <= C.S_CEILING, S
    m = _model(cfg, state)
    y1 = m(x.cuda())
    assert tuple(y1.shape) == tuple(a.shape) == (M, cfg["C"], T) and y1.dtype == torch.float32
    err = C.relrms(y1, a)
    print("conv-tasnet %s: S = %.3e, device = %.3e" % (name, S, err))
    assert err <= 2 * S, (err, S)
    assert not y1[..., -(cfg["L"] // 2):].any()  # the model's pad
    y2 = m(x.cuda())
    assert torch.equal(y1, y2)  # no atomics, fixed-order statistics: the same bits
    if M > 1:  # an utterance alone against itself inside the batch
        alone = m(x[1:2].cuda())
        assert C.relrms(alone[0], y1[1]) <= 2 * S
        assert C.relrms(alone[0], a[1]) <= 2 * S


def test_model_true_overlap(torch, model_refs):
    cfg, M, T, _ = CASES["small"]
    state, x, _, S = model_refs["small"]
    a = C.forward(state, cfg, x, overlap="true")
    y = _model(cfg, state, overlap="true")(x.cuda())
    err = C.relrms(y, a)
    print("conv-tasnet small, true overlap: S = %.3e, device = %.3e" % (S, err))
    assert y.shape == a.shape and err <= 2 * S, (err, S)
    assert bool(y[..., -(cfg["L"] // 2):].any())


def test_weights_loaded_after_a_forward_are_used(torch, model_refs):
    cfg, M, T, _ = CASES["small"]
    state, x, a, S = model_refs["small"]
    other = C.make_state(cfg, 77)
    m = _model(cfg, other)
    y0 = m(x.cuda())
    assert C.relrms(y0, a) > 0.5  # other weights, another output
    m.load_state_dict(state)
    assert m._prepared is None
    assert C.relrms(m(x.cuda()), a) <= 2 * S


def test_forward_refuses_bad_input(torch, model_refs):
    cfg = CASES["small"][0]
    m = _model(cfg, model_refs["small"][0])
    # a (1, T) view whose stride(0) is not T still counts as contiguous: same bits as the plain tensor
    x = model_refs["small"][1][:1].cuda()
    view = torch.as_strided(x, (1, x.shape[1]), (1, 1))  # (what torch.randn(T, 1).t() looks like)
    assert view.is_contiguous() and view.stride(0) != x.shape[1]
    assert torch.equal(m(view), m(x))
    with pytest.raises(ValueError):
        m(x.cpu())
    with pytest.raises(ValueError):
        m(torch.zeros(3010, device="cuda"))
    with pytest.raises(ValueError):
        m(torch.zeros((1, 10), device="cuda"))


# ---- the evaluation script ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eval_setup(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("tasnet_eval"))
    C.make_dataset(root, [5000, 13000, 3000, 9000])  # 13000 -> 4 segments, 9000 -> 3, 5000 -> 2, 3000 dropped: 9 = 8 + 1
    return {"data_dir": root, "eval_batch_size": 4, "sample_rate": 8000, "segment": 0.5, "cal_sdr": 0}


def test_eval_with_a_stand_in_model(torch, eval_setup):
    """The stand-in returns the two sources swapped plus a fixed small noise: the reordering must undo the swap, and each printed
    SI-SNRi is the host float64 value of (source + noise) to 1e-3 dB."""
    from mindaudio_amd.conv_tasnet import DatasetGenerator
    from mindaudio_amd.conv_tasnet.eval import evaluate
    from mindaudio_amd.metric import cal_SISNRi

    ds = DatasetGenerator(eval_setup["data_dir"], 4, segment=0.5, log=lambda s: None)
    assert len(ds) == 9
    noise = (1e-2 * np.random.RandomState(9).randn(2, 4000)).astype(np.float32)
    calls = []

    def stand_in(mixture):
        first = 8 * len(calls)
        calls.append(tuple(mixture.shape))
        src = np.stack([ds[i][2] for i in range(first, first + mixture.shape[0])])
        return torch.from_numpy((src + noise)[:, ::-1].copy()).to(mixture.device)

    lines = []
    avg, vals = evaluate(eval_setup, model=stand_in, log=lines.append)
    assert calls == [(8, 4000), (1, 4000)] and len(vals) == 9
    want = [cal_SISNRi(ds[i][2], ds[i][2] + noise, ds[i][0]) for i in range(9)]
    assert np.abs(np.array(vals) - want).max() <= 1e-3
    assert [ln for ln in lines if ln.startswith("Utt")] == ["Utt %d" % (i + 1) for i in range(9)]
    assert [ln for ln in lines if ln.startswith("\tSI-SNRi=")] == ["\tSI-SNRi=%.2f" % v for v in vals]
    assert lines[-1] == "Average SISNR improvement: %.2f" % avg and avg == pytest.approx(np.mean(want), abs=1e-3)


def test_eval_with_a_real_model(torch, eval_setup):
    from mindaudio_amd.conv_tasnet import DatasetGenerator
    from mindaudio_amd.conv_tasnet.eval import evaluate
    from mindaudio_amd.loss import Convtasnet_Loss
    from mindaudio_amd.metric import cal_SISNRi

    cfg = dict(C.SMALL, X=4, R=1)
    m = _model(cfg, C.make_state(cfg, 21))
    lines = []
    avg, vals = evaluate(eval_setup, model=m, log=lines.append)
    ds = DatasetGenerator(eval_setup["data_dir"], 4, segment=0.5, log=lambda s: None)
    assert len(vals) == len(ds) == 9 and len([ln for ln in lines if ln.startswith("Utt")]) == 9
    want = []
    for first in (0, 8):
        idx = range(first, min(first + 8, 9))
        mix = torch.from_numpy(np.stack([ds[i][0] for i in idx])).cuda()
        src = torch.from_numpy(np.stack([ds[i][2] for i in idx])).cuda()
        est = m(mix)
        assert est.shape == src.shape
        _, _, _, reordered = Convtasnet_Loss()(src, est, torch.tensor([4000] * len(idx)))
        for j, i in enumerate(idx):
            want.append(cal_SISNRi(ds[i][2], reordered[j].cpu().numpy(), ds[i][0]))
    assert np.allclose(vals, want, rtol=0, atol=1e-9)  # the same launches on the same inputs: the same bits
    assert lines[-1] == "Average SISNR improvement: %.2f" % (sum(want) / 9)
