"""GPU: Conv-TasNet training - every new kernel alone against float64 on seeded float32 inputs (guard words around every output),
the whole chain in the float32 validation mode and in bf16 mode against the autograd forms of conv_tasnet_train_cases.py, run-to-run
and batch-to-single bit equality, learning on one batch, and the train script with its checkpoint round trip.

Float32 tolerances come from the reference alone: MARGIN (4) x the error of the same piece evaluated in float32 on the CPU against
float64, plus one float32 ulp of the output's rms; the margin covers summation order.

bf16 mode, measured on the CPU (form (c) against form (a), TINY cases): S per group 0.011 (basis_signals) .. 0.156 (R = 2),
cosine over all parameters 0.9901 .. 0.9956 - above 0.99, so the cosine bound stays at the issue's 0.98."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_tasnet_cases as C  # noqa: E402
import conv_tasnet_train_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    from mindaudio_amd import _host, _lib

    _host.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


class Guarded:
    """An output buffer between two runs of guard words; `ok()` after the launch says they are untouched."""

    def __init__(self, shape, dev, dtype=torch.float32):
        n = int(np.prod(shape))
        self.flat = torch.full((n + 2 * GUARD,), 7.0, dtype=dtype, device=dev)
        self.flat[GUARD:GUARD + n] = -3.0  # (neither 0 nor a guard: an unwritten element shows)
        self.t = self.flat[GUARD:GUARD + n].view(shape)
        self.n = n

    def ptr(self):
        return self.t.data_ptr()

    def ok(self):
        return bool((self.flat[:GUARD] == 7.0).all() and (self.flat[GUARD + self.n:] == 7.0).all())


def rms(x):
    return float(torch.as_tensor(x).double().pow(2).mean().sqrt())


def within(got, ref64, ref32, what):
    """rms(got - ref64) <= MARGIN rms(ref32 - ref64) + ulp rms(ref64); prints the figures first."""
    got, ref64, ref32 = (torch.as_tensor(t).double().cpu() for t in (got, ref64, ref32))
    err, allowed = rms(got - ref64), T.MARGIN * rms(ref32 - ref64) + ULP * rms(ref64)
    print("%s: rms error %.3e, allowed %.3e (rms %.3e)" % (what, err, allowed, rms(ref64)))
    assert err <= allowed, (what, err, allowed)


def seeded(shape, seed, scale=1.0):
    return (scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).float()


def ck(rc):
    assert rc == 0, rc


def sync():
    torch.cuda.synchronize()


# ---- loss gradient ------------------------------------------------------------------------------------------------------------------
def test_si_snr_grad(lib, dev):
    B, Cs, n = 2, 2, 1510
    src, est = seeded((B, Cs, n), 1), seeded((B, Cs, n), 2)
    est = est + 0.5 * src[:, [0, 1]] * torch.tensor([1.0, 0.0])[None, :, None] + 0.1  # some correlation, a mean to remove
    lengths, perms = [n, n - 137], [(0, 1), (1, 0)]
    ref64 = T.si_snr_grad_closed(src, est, lengths, perms)

    e32 = est.clone().requires_grad_(True)
    table = T.si_snr_table(src, e32, lengths)
    (-sum(table[b, perms[b][j], j] for b in range(B) for j in range(Cs)) / (B * Cs)).backward()
    out = Guarded((B, Cs, n), dev)
    d = [t.to(dev) for t in (src, est)]
    lens, perm = torch.tensor(lengths, device=dev), torch.tensor(perms, dtype=torch.int64, device=dev)
    ck(lib.ma_si_snr_grad_f32(d[0].data_ptr(), d[1].data_ptr(), lens.data_ptr(), perm.data_ptr(), B, Cs, n, out.ptr(), None))
    sync()
    assert out.ok()
    within(out.t, ref64, e32.grad, "si_snr_grad")
    assert not out.t[1, :, n - 137:].any() and out.t[1, :, :n - 137].abs().min() > 0  # exactly 0.0 beyond the length


# ---- decoder / mask backward -------------------------------------------------------------------------------------------------------
def _decode_ref(score, mw, basis, d_out, overlap, dtype, M, K, Cs, N):
    sc = score.to(dtype).clone().requires_grad_(True)
    w = mw.to(dtype).clone().requires_grad_(True)
    bs = basis.to(dtype).clone().requires_grad_(True)
    s4 = sc.view(M, K, Cs, N).permute(0, 2, 1, 3)
    frames = (w.view(M, 1, K, N) * F.relu(s4)) @ bs.t()
    out = C.overlap_paired(frames) if overlap == "paired" else C.overlap_true(frames)
    (out * d_out.to(dtype)).sum().backward()
    return sc.grad, w.grad, bs.grad


@pytest.mark.parametrize("overlap", ["paired", "true"])
def test_decode_bwd(lib, dev, overlap):
    M, K, Cs, N, L = 2, 150, 2, 64, 20
    score, mw = seeded((M * K, Cs * N), 3), seeded((M * K, N), 4).abs()
    basis, d_out = seeded((L, N), 5, 0.3), seeded((M, Cs, (K + 1) * (L // 2)), 6)
    ref64 = _decode_ref(score, mw, basis, d_out, overlap, torch.float64, M, K, Cs, N)
    ref32 = _decode_ref(score, mw, basis, d_out, overlap, torch.float32, M, K, Cs, N)
    G = lib.ma_tasnet_decode_bwd_parts(K, Cs, N, L)
    assert G == 5  # 19 chunks of 8 frames, 4 per workgroup: the last workgroup walks 3
    ds, dm, db = Guarded((M * K, Cs * N), dev), Guarded((M * K, N), dev), Guarded((M * G, L, N), dev)
    d = [t.to(dev) for t in (d_out, score, mw, basis)]
    ck(lib.ma_tasnet_decode_bwd_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), M, K, Cs, N, d[3].data_ptr(), L,
                                    0 if overlap == "paired" else 1, ds.ptr(), dm.ptr(), db.ptr(), None))
    sync()
    assert ds.ok() and dm.ok() and db.ok()
    within(ds.t, ref64[0], ref32[0], "d_score")
    within(dm.t, ref64[1], ref32[1], "d_mixture_w")
    within(db.t.sum(0), ref64[2], ref32[2], "d_basis")
    assert not ds.t[score.to(dev) <= 0].any()  # the mask's gradient is exactly 0 where the ReLU is off


# ---- gLN backward with PReLU (launches (a) and (c)) -----------------------------------------------------------------------------------
def _gln_prelu_ref(y0, a, du, dtype, M, K, H):
    y = y0.to(dtype).view(M, K, H).transpose(1, 2).clone().requires_grad_(True)
    s = torch.tensor([a], dtype=dtype, requires_grad=True)
    (T.gln(F.prelu(y, s)) * du.to(dtype).view(M, K, H).transpose(1, 2)).sum().backward()
    return y.grad.transpose(1, 2).reshape(M * K, H), s.grad


@pytest.mark.parametrize("K", [64, 150])
def test_gln_prelu_bwd(lib, dev, K):
    M, H, a = 2, 128, 0.21
    y0, du = seeded((M * K, H), 7) + 0.3, seeded((M * K, H), 8)
    y0[K:] *= 2.5  # utterances with different statistics
    ref64, ref32 = _gln_prelu_ref(y0, a, du, torch.float64, M, K, H), _gln_prelu_ref(y0, a, du, torch.float32, M, K, H)
    P = lib.ma_tasnet_stat_parts(K, H)
    assert P == (K + 63) // 64
    yd, dud, ad = y0.to(dev), du.to(dev), torch.tensor([a], device=dev)
    p1 = torch.empty_like(yd)
    part = torch.empty(M * P * 3, dtype=torch.float64, device=dev)
    part2 = Guarded((M * P * 2,), dev, torch.float64)
    out, outb, da = Guarded((M * K, H), dev), Guarded((M * K, H), dev, torch.bfloat16), Guarded((M * P,), dev)
    da2 = Guarded((M * P,), dev)
    ck(lib.ma_prelu_gln_stats(yd.data_ptr(), M, K, H, ad.data_ptr(), p1.data_ptr(), part.data_ptr(), None))
    ck(lib.ma_gln_bwd_stats(dud.data_ptr(), yd.data_ptr(), M, K, H, part.data_ptr(), ad.data_ptr(), part2.ptr(), None))
    ck(lib.ma_gln1_bwd(dud.data_ptr(), yd.data_ptr(), M, K, H, part.data_ptr(), part2.ptr(), ad.data_ptr(), out.ptr(), 0, da.ptr(), None))
    ck(lib.ma_gln1_bwd(dud.data_ptr(), yd.data_ptr(), M, K, H, part.data_ptr(), part2.ptr(), ad.data_ptr(), outb.ptr(), 1, da2.ptr(), None))
    sync()
    assert part2.ok() and out.ok() and outb.ok() and da.ok() and da2.ok()
    within(out.t, ref64[0], ref32[0], "d_y0")
    got = float(da.t.double().sum())
    print("d_slope: got %.9g, float64 %.9g, float32 %.9g" % (got, float(ref64[1]), float(ref32[1])))
    assert abs(got - float(ref64[1])) <= T.MARGIN * abs(float(ref32[1]) - float(ref64[1])) + ULP * abs(float(ref64[1]))
    assert torch.equal(outb.t, out.t.to(torch.bfloat16)) and torch.equal(da.t, da2.t)  # the bf16 operand is the float32 one, rounded


# ---- depthwise backward (launches (a) and (b)) ----------------------------------------------------------------------------------------
def _dw_ref(y0, a1, w, a2, dh, dil, dtype, M, K, H):
    y = y0.to(dtype).view(M, K, H).transpose(1, 2)
    n1 = T.gln(F.prelu(y, torch.tensor([a1], dtype=dtype))).detach().requires_grad_(True)
    ww = w.to(dtype).clone().requires_grad_(True)
    s = torch.tensor([a2], dtype=dtype, requires_grad=True)
    h = T.gln(F.prelu(T.dwconv(n1, ww, dil), s))
    (h * dh.to(dtype).view(M, K, H).transpose(1, 2)).sum().backward()
    return n1.grad.transpose(1, 2).reshape(M * K, H), ww.grad, s.grad


@pytest.mark.parametrize("K", [100, 150])
@pytest.mark.parametrize("dil", [1, 64, 128])
def test_depthwise_bwd(lib, dev, dil, K):
    M, H, a1, a2 = 2, 128, 0.23, 0.27
    y0, dh, w = seeded((M * K, H), 9) + 0.2, seeded((M * K, H), 10), seeded((H, 1, 3), 11, 0.6)
    ref64, ref32 = (_dw_ref(y0, a1, w, a2, dh, dil, dt, M, K, H) for dt in (torch.float64, torch.float32))
    P = lib.ma_tasnet_stat_parts(K, H)
    yd, dhd = y0.to(dev), dh.to(dev)
    wt = w.squeeze(1).t().contiguous().to(dev)  # (3, H)
    s1, s2 = torch.tensor([a1], device=dev), torch.tensor([a2], device=dev)
    p1 = torch.empty_like(yd)
    pa, pb, pb_inf = (torch.empty(M * P * 3, dtype=torch.float64, device=dev) for _ in range(3))
    d0, z, z_inf = Guarded((M * K, H), dev), Guarded((M * K, H), dev), torch.empty_like(yd)
    p2h = torch.empty(M * P * 2, dtype=torch.float64, device=dev)
    du, p2u, da2, dwp = Guarded((M * K, H), dev), Guarded((M * P * 2,), dev, torch.float64), Guarded((M * P,), dev), Guarded((M * P, 3, H), dev)
    ck(lib.ma_prelu_gln_stats(yd.data_ptr(), M, K, H, s1.data_ptr(), p1.data_ptr(), pa.data_ptr(), None))
    ck(lib.ma_gln_dwconv_prelu_train(p1.data_ptr(), M, K, H, pa.data_ptr(), wt.data_ptr(), 3, dil, s2.data_ptr(), d0.ptr(), z.ptr(),
                                     pb.data_ptr(), None))
    ck(lib.ma_gln_dwconv_prelu(p1.data_ptr(), M, K, H, pa.data_ptr(), wt.data_ptr(), 3, dil, s2.data_ptr(), z_inf.data_ptr(),
                               pb_inf.data_ptr(), None))
    ck(lib.ma_gln_bwd_stats(dhd.data_ptr(), d0.ptr(), M, K, H, pb.data_ptr(), s2.data_ptr(), p2h.data_ptr(), None))
    ck(lib.ma_gln2_bwd_dwconv(dhd.data_ptr(), d0.ptr(), yd.data_ptr(), M, K, H, pa.data_ptr(), pb.data_ptr(), p2h.data_ptr(),
                              s1.data_ptr(), s2.data_ptr(), wt.data_ptr(), 3, dil, du.ptr(), p2u.ptr(), da2.ptr(), dwp.ptr(), None))
    sync()
    assert d0.ok() and z.ok() and du.ok() and p2u.ok() and da2.ok() and dwp.ok()
    # the training forward is the inference kernel plus one store: the same bits
    assert torch.equal(z.t, z_inf) and torch.equal(pb, pb_inf)
    assert torch.equal(torch.where(d0.t >= 0, d0.t, a2 * d0.t), z.t)
    within(du.t, ref64[0], ref32[0], "d_u dil %d" % dil)
    within(dwp.t.sum(0).t().reshape(H, 1, 3), ref64[1], ref32[1], "d_taps dil %d" % dil)
    if dil >= K:  # the outer taps never land: their gradient is exactly 0
        assert not dwp.t[:, 0].any() and not dwp.t[:, 2].any()
    got = float(da2.t.double().sum())
    print("d_slope2: got %.9g, float64 %.9g, float32 %.9g" % (got, float(ref64[2]), float(ref32[2])))
    assert abs(got - float(ref64[2])) <= T.MARGIN * abs(float(ref32[2]) - float(ref64[2])) + ULP * abs(float(ref64[2]))
    # the partials of the next gLN backward are the sums of d_u and d_u * xhat1
    n1 = T.gln(F.prelu(y0.double().view(M, K, H), torch.tensor([a1], dtype=torch.float64)).transpose(1, 2)).transpose(1, 2)
    want = torch.stack([ref64[0].view(M, K, H).sum(dim=(1, 2)), (ref64[0].view(M, K, H) * n1).sum(dim=(1, 2))], dim=1)
    got2 = p2u.t.view(M, P, 2).sum(1).cpu()
    scale = float((ref64[0].view(M, K, H) * n1).abs().sum(dim=(1, 2)).max())
    assert (got2 - want).abs().max() <= 1e-5 * scale


# ---- encoder backward ------------------------------------------------------------------------------------------------------------------
def _enc_ref(x, U, dnb, dmw, dtype, M, K, N, L):
    u = U.to(dtype).clone().requires_grad_(True)
    mw = F.relu(F.conv1d(x.to(dtype)[:, None, :], u, stride=L // 2))  # (M, N, K)
    t = lambda v: v.to(dtype).view(M, K, N).transpose(1, 2)  # noqa: E731
    ((T.gln(mw) * t(dnb)).sum() + (mw * t(dmw)).sum()).backward()
    return u.grad


def test_encode_bwd(lib, dev):
    M, K, N, L = 2, 150, 64, 20
    n = T.samples(K)
    x, U = seeded((M, n), 12, 0.1), seeded((N, 1, L), 13, 0.5)
    dnb, dmw = seeded((M * K, N), 14), seeded((M * K, N), 15)
    ref64, ref32 = (_enc_ref(x, U, dnb, dmw, dt, M, K, N, L) for dt in (torch.float64, torch.float32))
    P, G = lib.ma_tasnet_stat_parts(K, N), lib.ma_tasnet_encode_bwd_parts(K, N, L)
    assert G == 3  # 10 chunks of 16 frames, 4 per workgroup: the last workgroup walks 2, its last chunk 6 frames
    xd, ut, dnbd, dmwd = x.to(dev), U.squeeze(1).t().contiguous().to(dev), dnb.to(dev), dmw.to(dev)
    mw = torch.empty((M * K, N), device=dev)
    part, p2 = torch.empty(M * P * 3, dtype=torch.float64, device=dev), torch.empty(M * P * 2, dtype=torch.float64, device=dev)
    one = torch.ones(4, device=dev)
    out = Guarded((M * G, L, N), dev)
    ck(lib.ma_tasnet_encode_f32(xd.data_ptr(), M, n, n, ut.data_ptr(), L, N, mw.data_ptr(), part.data_ptr(), None))
    ck(lib.ma_gln_bwd_stats(dnbd.data_ptr(), mw.data_ptr(), M, K, N, part.data_ptr(), one.data_ptr(), p2.data_ptr(), None))
    ck(lib.ma_tasnet_encode_bwd_f32(xd.data_ptr(), M, n, n, mw.data_ptr(), part.data_ptr(), dnbd.data_ptr(), p2.data_ptr(), dmwd.data_ptr(), L, N,
                                    out.ptr(), None))
    sync()
    assert out.ok()
    within(out.t.sum(0).t().reshape(N, 1, L), ref64, ref32, "d_U")


# ---- SGD ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_update(lib, dev, momentum):
    n, lr, wd = 1000, 0.05, 0.01
    p0 = seeded((n,), 16)
    ref = {f: {"p": p0.to(f).clone()} for f in (torch.float64, torch.float32)}
    bufs = {f: {} for f in ref}
    p, buf, mirror = Guarded((n,), dev), Guarded((n,), dev), Guarded((n,), dev, torch.bfloat16)
    p.t.copy_(p0)
    for step in range(3):
        g = seeded((n,), 20 + step)
        for f in ref:
            T.sgd_step(ref[f], {"p": g.to(f)}, bufs[f], lr, momentum, wd)
        gd = g.to(dev)
        ck(lib.ma_sgd_momentum_f32(p.ptr(), gd.data_ptr(), buf.ptr() if momentum else None, n, lr, momentum, wd, 1 if step == 0 else 0,
                                   mirror.ptr(), None))
    sync()
    assert p.ok() and buf.ok() and mirror.ok()
    within(p.t, ref[torch.float64]["p"], ref[torch.float32]["p"], "sgd")
    assert torch.equal(mirror.t, p.t.to(torch.bfloat16))
    before = p.t.clone()
    ck(lib.ma_sgd_momentum_f32(p.ptr(), gd.data_ptr(), buf.ptr() if momentum else None, n, 0.0, momentum, wd, 0, None, None))
    sync()
    assert torch.equal(p.t, before)  # lr = 0 leaves the parameters bit-identical


# ---- whole chain -----------------------------------------------------------------------------------------------------------------------
def _trainer(name, dev, operands, momentum=0.9, weight_decay=0.01):
    from mindaudio_amd.models import ConvTasNet, ConvTasNetTrainer

    c = T.case(name)
    model = ConvTasNet(**c["cfg"], overlap=c["overlap"])
    model.load_state_dict(c["state"])
    model.to(dev)
    tr = ConvTasNetTrainer(model, momentum=momentum, weight_decay=weight_decay, operands=operands)
    return c, tr, (c["mixture"].to(dev), c["sources"].to(dev), c["lengths"])


@pytest.mark.parametrize("name", list(T.CASES))
def test_chain_f32(dev, name):
    c, tr, batch = _trainer(name, dev, "f32")
    la, ga, aa = T.reference(name, "a")
    lb, gb, _ = T.reference(name, "b")
    loss = tr.loss_and_grads(*batch)
    got = {k: v.cpu() for k, v in tr.gradients().items()}
    G, A, Bf = T.groups(got), T.groups(ga), T.groups(gb)
    for k in A:
        print("%s: relrms %.3e, (b) %.3e" % (k, C.relrms(G[k], A[k]), C.relrms(Bf[k], A[k])))
    assert T.check_f32(got, ga, gb) == []
    d_est = tr.activation_gradients()["estimate"].cpu()
    if name == "ragged":
        assert not d_est[1, :, c["lengths"][1]:].any()
    steps, lr = 5, 1e-3
    args = (c["state"], c["cfg"], c["mixture"], c["sources"], c["lengths"], c["overlap"])
    ta, tb = (T.trajectory(*args, form, steps, lr, 0.9, 0.01) for form in ("a", "b"))
    losses = [loss] + [0.0] * steps
    for i in range(steps):
        value = tr.step(*batch, lr)
        losses[i] = value
    losses[steps] = tr.loss_and_grads(*batch)
    for i in range(steps + 1):
        allowed = T.MARGIN * abs(tb[i] - ta[i]) + 1e-6
        print("step %d: loss %.8f, (a) %.8f, (b) %.8f, allowed %.2e" % (i, losses[i], ta[i], tb[i], allowed))
        assert abs(losses[i] - ta[i]) <= allowed, (i, losses[i], ta[i], allowed)


@pytest.mark.parametrize("name", list(T.CASES))
def test_chain_bf16(dev, name):
    """Per parameter group relrms(device, (a)) <= 2 S with S = relrms((c), (a)) <= 0.2, and the cosine over all parameters >= 0.98
    (form (c)'s own cosine, measured on the CPU: 0.9901 .. 0.9956)."""
    c, tr, batch = _trainer(name, dev, "bf16")
    _, ga, _ = T.reference(name, "a")
    _, gc, _ = T.reference(name, "c")
    tr.loss_and_grads(*batch)
    got = {k: v.cpu() for k, v in tr.gradients().items()}
    A, Cc, G = T.by_kind(ga), T.by_kind(gc), T.by_kind(got)
    for k in A:
        print("%s: relrms %.4f, S %.4f" % (k, C.relrms(G[k], A[k]), C.relrms(Cc[k], A[k])))
    bad, cos = T.check_bf16(got, ga, gc)
    print("cosine %.5f, (c) %.5f" % (cos, T.cosine(gc, ga)))
    assert bad == [] and cos >= T.COS_MIN


@pytest.mark.parametrize("operands", ["f32", "bf16"])
def test_same_bits_from_run_to_run(dev, operands):
    c, tr, batch = _trainer("k150", dev, operands)
    l1 = tr.loss_and_grads(*batch)
    g1 = {k: v.clone() for k, v in tr.gradients().items()}
    a1 = {k: v.clone() for k, v in tr.activation_gradients().items()}
    l2 = tr.loss_and_grads(*batch)
    assert l1 == l2
    for k, v in tr.gradients().items():
        assert torch.equal(v, g1[k]), k
    for k, v in tr.activation_gradients().items():
        assert torch.equal(v, a1[k]), k


def test_utterances_do_not_see_each_other(dev):
    """Float32 operands (one summation order whatever the row count).  Changing utterance 1's data leaves utterance 0's activation
    gradients bit-identical; a batch of 2 equals the two utterances run alone after scaling by the mean - exactly in the activation
    gradients (the factor is 2), to the float32 sum in the parameter gradients."""
    c, tr, (mix, src, lengths) = _trainer("k100", dev, "f32")
    K = c["K"]
    tr.loss_and_grads(mix, src, lengths)
    both = {k: v.clone() for k, v in tr.activation_gradients().items()}
    gboth = {k: v.cpu().clone() for k, v in tr.gradients().items()}
    mix2, src2 = mix.clone(), src.clone()
    mix2[1] = mix[1].flip(0) * 1.5
    src2[1] = src[1].flip(1)
    tr.loss_and_grads(mix2, src2, lengths)
    for k, v in tr.activation_gradients().items():
        rows = 1 if k == "estimate" else K
        assert torch.equal(v[:rows], both[k][:rows]), k
        assert not torch.equal(v[rows:], both[k][rows:]), k
    total = None
    for m in range(2):
        tr.loss_and_grads(mix[m:m + 1], src[m:m + 1], lengths[m:m + 1])
        for k, v in tr.activation_gradients().items():
            rows = 1 if k == "estimate" else K
            assert torch.equal(v * 0.5, both[k][m * rows:(m + 1) * rows]), (k, m)
        g = {k: v.cpu().double() for k, v in tr.gradients().items()}
        total = g if total is None else {k: total[k] + g[k] for k in g}
    _, ga, _ = T.reference("k100", "a")
    _, gb, _ = T.reference("k100", "b")
    G, W, A, Bf = T.groups({k: v / 2 for k, v in total.items()}), T.groups(gboth), T.groups(ga), T.groups(gb)
    for k in W:
        assert C.relrms(G[k], W[k]) <= T.MARGIN * C.relrms(Bf[k], A[k]), k


def test_it_learns(dev):
    """30 steps on one TINY batch in bf16 mode lower the loss by at least half of what form (a)'s own 30 steps gain."""
    c, tr, batch = _trainer("k64", dev, "bf16")
    steps, lr = 30, 1e-3
    ta = T.trajectory(c["state"], c["cfg"], c["mixture"], c["sources"], c["lengths"], c["overlap"], "a", steps, lr, 0.9, 0.01)
    gain = ta[0] - ta[-1]
    assert gain > 0
    first = tr.step(*batch, lr)
    for _ in range(steps - 1):
        tr.step(*batch, lr)
    last = tr.loss_and_grads(*batch)
    print("loss %.5f -> %.5f; form (a) %.5f -> %.5f" % (first, last, ta[0], ta[-1]))
    assert first - last >= 0.5 * gain


# ---- script ------------------------------------------------------------------------------------------------------------------------------
def test_train_script_checkpoint_eval_resume(dev, tmp_path):
    import mindaudio_amd.conv_tasnet.eval as ev
    import mindaudio_amd.conv_tasnet.train as script
    from mindaudio_amd.models import ConvTasNet
    from mindaudio_amd.utils import ckpt

    data = tmp_path / "data"
    C.make_dataset(str(data), [4000, 4100, 4000])
    cfg = dict(T.TINY, X=2, device_num=1, causal=0, max_norm=0, norm_type="gLN", mask_nonlinear="relu", train_dir=str(data), data_dir=str(data),
               batch_size=2, eval_batch_size=2, sample_rate=8000, segment=0.5, epochs=2, l2=0.01, momentum=0.9, continue_train=0,
               save_folder=str(tmp_path / "exp"), cal_sdr=0, optimizer="adam", lr=0.0003)
    lines = []
    torch.manual_seed(0)
    losses = script.train(cfg, log=lines.append)
    assert len(losses) == 4 and all(np.isfinite(losses))  # 4 segments (4100 gives two), 2 a step, 2 epochs
    assert [ln for ln in lines if ln.startswith("epoch: 2 step: 2, loss is ")]
    saved = sorted(os.listdir(cfg["save_folder"]))
    assert saved == ["Conv-TasNet-2_2.ckpt"]  # keep_checkpoint_max = 1
    path = os.path.join(cfg["save_folder"], saved[0])
    model = ConvTasNet(*(cfg[k] for k in "NLBHPXRC"))
    missing, unexpected = ckpt.load_mindspore_checkpoint(model, path)
    assert missing == [] and unexpected == []
    average, values = ev.evaluate(dict(cfg, model_path=path), log=lambda s: None)
    assert len(values) == 4 and np.isfinite(average)
    resumed = script.train(dict(cfg, continue_train=1, ckpt_path=path, epochs=1, save_folder=str(tmp_path / "exp2")), log=lines.append)
    assert len(resumed) == 2 and all(np.isfinite(resumed))
    assert abs(resumed[0] - losses[0]) > 0  # it started from the trained weights, not from a fresh initialisation
