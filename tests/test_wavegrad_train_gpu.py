"""GPU: WaveGrad training (csrc/wavegrad_train.hip, models/wavegrad_train.py, wavegrad/train.py).

Kernels, each against float64 of the same float32 inputs.  Where the arithmetic allows it the data are small dyadic integers (scale 1,
shift 0, a loss scale of B T so that g = +-1) and the comparison is exact; elsewhere the bound is written beside the assertion, in
units of u = 2^-24 times the magnitude sum of the same expression.  Products (dW by taps, dX through the reversed weights, the
kernel = stride backward) run on small integers, exact in bf16 and in the float32 accumulators.

Chain: wavegrad_train_cases.py holds the reference (torch.autograd in forms (a) float64, (b) float32, (c) bf16 operands).
  float32 mode  every cell (weight and bias) within MARGIN (4) x form (b)'s own error of form (a); the loss over 5 steps the same.
  bf16 mode     per parameter group relrms(device, a) <= 2 S, S = relrms(c, a) <= 0.2; cosine >= 0.98.
The measured figures are printed by the tests and recorded in DESIGN.md."""
import math
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import wavegrad_cases as C  # noqa: E402
import wavegrad_train_cases as T  # noqa: E402

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


def _ptr(t):
    return t.data_ptr() if t is not None else None


def ints(torch, shape, seed, lo=-3, hi=4, nonzero=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi, shape, generator=g).float()
    if nonzero:
        v = torch.where(v == 0, torch.ones_like(v), v)
    return v


def guarded(torch, t):
    """A device copy with one NaN guard row of 64 floats behind it; -> (view, whole)."""
    whole = torch.full((t.numel() + 64,), float("nan"), device="cuda")
    whole[:t.numel()] = t.reshape(-1).cuda()
    return whole[:t.numel()].view(t.shape), whole


def guard_intact(torch, whole, n):
    return bool(torch.isnan(whole[n:]).all())


def reduce_parts(torch, lib, part, stride, splits, pieces):
    """ma_reduce_splits_batch_f32 over per-workgroup partials: pieces = [(offset, count)] -> list of float32 tensors."""
    from mindaudio_amd.train import plans

    outs = [torch.full((n,), float("nan"), device="cuda") for _, n in pieces]
    items = [plans._reduce_item(part.data_ptr() + off * 4, o, n, n, n, splits, stride, splits >= 64, accumulate=False)
             for (off, n), o in zip(pieces, outs)]
    table = plans.ItemTable(items, "cuda")
    _ok(lib.ma_reduce_splits_batch_f32(*table.args, None))
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


# ---- L1 loss + last_conv backward ------------------------------------------------------------------------------------------------------
def _l1_last(torch, lib, pred, noise, x, w, scale):
    B, Tn, Cc = x.shape
    taps = w.shape[0]
    parts = lib.ma_wavegrad_last_bwd_parts(B, Tn)
    stride = (taps * Cc + 1 + 7) // 8 * 8
    g, gw = guarded(torch, torch.zeros(B, Tn))
    dx, dxw = guarded(torch, torch.zeros(B, Tn, Cc))
    part = torch.full((parts * stride,), float("nan"), device="cuda")
    lp, loss = torch.zeros(parts, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    pd, nd, xd, wd = pred.cuda(), noise.cuda(), x.contiguous().cuda(), w.contiguous().cuda()
    _ok(lib.ma_wavegrad_l1_last_bwd_f32(pd.data_ptr(), nd.data_ptr(), xd.data_ptr(), B, Tn, Cc, wd.data_ptr(), taps, scale, g.data_ptr(),
                                        dx.data_ptr(), part.data_ptr(), stride, lp.data_ptr(), loss.data_ptr(), None))
    dw, db = reduce_parts(torch, lib, part, stride, parts, [(0, taps * Cc), (taps * Cc, 1)])
    assert guard_intact(torch, gw, g.numel()) and guard_intact(torch, dxw, dx.numel())
    return float(loss[0].item()), g.cpu(), dx.cpu(), dw.view(taps, Cc), db


@pytest.mark.parametrize("Tn", [3, 65])
@pytest.mark.parametrize("Cc", [8, 128])
@pytest.mark.parametrize("taps", [3, 7])
def test_l1_last_bwd(torch, lib, Tn, Cc, taps):
    """Integers and loss_scale = B T (g = +-1, or 0 where pred == noise): g, dx, dw and db exact.  The loss is a float64 sum of
    float32 |differences| in another order than the reference's: within B T 2^-52 relative."""
    B = 2
    F = torch.nn.functional
    pred, noise = ints(torch, (B, Tn), 1, -5, 6), ints(torch, (B, Tn), 2, -5, 6) + 0.5
    noise[1, Tn // 2] = pred[1, Tn // 2]  # sign(0) = 0
    x, w = ints(torch, (B, Tn, Cc), 3), ints(torch, (taps, Cc), 4)
    loss, g, dx, dw, db = _l1_last(torch, lib, pred, noise, x, w, float(B * Tn))
    d = (pred - noise).double()
    want_g = torch.sign(d)
    assert float(want_g[1, Tn // 2]) == 0.0 and torch.equal(g.double(), want_g)
    ref_loss = float(d.abs().mean())
    assert abs(loss - ref_loss) <= B * Tn * 2.0 ** -52 * ref_loss
    half = taps // 2
    # dx[b, t, c] = sum_j g[b, t - (j - half)] w[j, c]: a transposed convolution = conv of g with the flipped taps
    want_dx = F.conv1d(want_g[:, None], w.double().t().flip(1)[:, None], padding=half).transpose(1, 2)
    assert torch.equal(dx.double(), want_dx)
    xp = F.pad(x.double(), (0, 0, half, half))
    want_dw = torch.stack([(want_g[:, :, None] * xp[:, j:j + Tn]).sum(dim=(0, 1)) for j in range(taps)])
    assert torch.equal(dw.double(), want_dw)
    assert float(db[0]) == float(want_g.sum())


def test_l1_last_bwd_scale(torch, lib):
    """A loss scale that is no multiple of B T: g is sign * float32(scale / (B T)) exactly, dx within (taps + 1) u of the magnitude sum."""
    B, Tn, Cc, taps, scale = 2, 65, 8, 3, 4096.0
    g0 = torch.Generator().manual_seed(5)
    pred, noise, x, w = (torch.randn(s, generator=g0) for s in ((B, Tn), (B, Tn), (B, Tn, Cc), (taps, Cc)))
    loss, g, dx, dw, db = _l1_last(torch, lib, pred, noise, x, w, scale)
    gs = torch.tensor(scale / (B * Tn), dtype=torch.float64).float()
    assert torch.equal(g, torch.sign(pred - noise) * gs)
    F = torch.nn.functional
    want = F.conv1d(g.double()[:, None], w.double().t().flip(1)[:, None], padding=1).transpose(1, 2)
    mag = F.conv1d(g.double().abs()[:, None], w.double().abs().t().flip(1)[:, None], padding=1).transpose(1, 2)
    assert float(((dx.double() - want).abs() / ((taps + 1) * U * mag)).max()) <= 1.0


# ---- producer backward -------------------------------------------------------------------------------------------------------------------
def _pack_bwd_ref(torch, dop, x, f, film, slope, mul, dres, res_mul, absolute=False):
    """float64 of the contract; absolute: the same expression on magnitudes (the error bound's scale).  -> (dx, dfilm or None)."""
    B, Tin, Cc = x.shape
    v = torch.repeat_interleave(x.double(), f, dim=1)
    g = torch.zeros_like(v)
    dfilm = None
    r2 = math.sqrt(2.0)
    if dop is not None:
        d = dop.double()[:, :, :Cc]
        if film is not None:
            sh, sc = film.double()[:, :, :Cc], film.double()[:, :, Cc:2 * Cc]
            pre = (sc * v + sh) / r2
        else:
            pre = v
        mask = torch.where(pre >= 0, torch.ones_like(pre), torch.full_like(pre, slope))
        g = d * mul * mask
        if absolute:
            g = g.abs()
        if film is not None:
            dfilm = torch.cat([g / r2, g * (v.abs() if absolute else v) / r2], dim=2)
            g = g * (sc.abs() if absolute else sc) / r2
    if dres is not None:
        g = g + (dres.double().abs() * abs(res_mul) if absolute else dres.double() * res_mul)
    return g.view(B, Tin, f, Cc).sum(2), dfilm


@pytest.mark.parametrize("f", [1, 2, 3, 5])
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("slope", [1.0, 0.2])
@pytest.mark.parametrize("res", [False, True])
def test_pack_bwd(torch, lib, f, film, slope, res):
    """Every variant the forward plan uses, with and without accumulation, T_in in {1, 9}, C = 8 under a row stride of 64 and C = 128.
    Without FiLM, with slope 1 and dyadic factors everything is a sum of small integers: exact.  Else each element is at most f + 7
    roundings of float32 (mul, mask, three FiLM factors, res_mul, f sums, the accumulation): (f + 7) u of the magnitude sum.  |pre|
    >= 0.25 by construction, so the mask is the float64 one."""
    exact = not film and slope == 1.0
    mul, res_mul = (0.5, 0.25) if exact else (1.0 / f, 1.0 / (f * math.sqrt(2.0)))
    for Tin, Cc, acc in [(1, 8, 0), (9, 8, 1), (9, 128, 0), (1, 128, 1)]:
        B, ld = 2, (Cc + 63) // 64 * 64
        To = Tin * f
        x = ints(torch, (B, Tin, Cc), 10 + Tin + Cc, nonzero=True)
        dop = torch.full((B, To, ld), float("nan"))
        dop[:, :, :Cc] = ints(torch, (B, To, Cc), 11)
        fm = None
        if film:
            g0 = torch.Generator().manual_seed(12)
            fm = torch.cat([torch.rand((B, To, Cc), generator=g0) * 0.5 - 0.25, torch.rand((B, To, Cc), generator=g0) + 0.5], dim=2)
        dres = ints(torch, (B, To, Cc), 13) if res else None
        dx0, df0 = ints(torch, (B, Tin, Cc), 14), ints(torch, (B, To, 2 * Cc), 15)
        dx, dxw = guarded(torch, dx0)
        df, dfw = guarded(torch, df0)
        xd, dd = x.cuda(), dop.cuda()
        fd, rd = (fm.cuda() if film else None), (dres.cuda() if res else None)
        _ok(lib.ma_wavegrad_pack_bwd_f32(dd.data_ptr(), ld, xd.data_ptr(), B, Tin, f, Cc, _ptr(fd), 2 * Cc if film else 0, slope, mul, _ptr(rd),
                                         res_mul, dx.data_ptr(), acc, df.data_ptr() if film else None, 2 * Cc if film else 0, acc, None))
        torch.cuda.synchronize()
        assert guard_intact(torch, dxw, dx.numel()) and guard_intact(torch, dfw, df.numel())
        want, wfilm = _pack_bwd_ref(torch, dop, x, f, fm, slope, mul, dres, res_mul)
        mag, mfilm = _pack_bwd_ref(torch, dop, x, f, fm, slope, mul, dres, res_mul, absolute=True)
        if acc:
            want, mag = want + dx0.double(), mag + dx0.double().abs()
        if exact:
            assert torch.equal(dx.cpu().double(), want), (Tin, Cc, acc)
        else:
            assert float(((dx.cpu().double() - want).abs() / ((f + 7) * U * mag + 1e-300)).max()) <= 1.0, (Tin, Cc, acc)
        if film:
            if acc:
                wfilm, mfilm = wfilm + df0.double(), mfilm + df0.double().abs()
            assert float(((df.cpu().double() - wfilm).abs() / (5 * U * mfilm + 1e-300)).max()) <= 1.0, (Tin, Cc, acc)  # mul, mask, v, 1/sqrt2, acc
        else:
            assert torch.equal(df.cpu(), df0)  # untouched
        if res and f > 1:  # the op without an operand output (block1 repeated): dop NULL
            dx2, dx2w = guarded(torch, dx0)
            _ok(lib.ma_wavegrad_pack_bwd_f32(None, 0, xd.data_ptr(), B, Tin, f, Cc, None, 0, 1.0, 1.0, rd.data_ptr(), 0.25, dx2.data_ptr(), 0,
                                             None, 0, 0, None))
            torch.cuda.synchronize()
            assert torch.equal(dx2.cpu().double(), (dres.double() * 0.25).view(B, Tin, f, Cc).sum(2)) and guard_intact(torch, dx2w, dx2.numel())


def test_pack_bwd_mask_is_the_forwards(torch, lib):
    """The LeakyReLU mask comes from the forward's own value: fma(scale, v, shift) / sqrt 2 recomputed bit for bit.  Elements whose
    float32 fma is exactly zero or of the smallest magnitudes take the side the forward's producer took (its output's sign bit)."""
    B, Tn, Cc = 1, 64, 64
    g0 = torch.Generator().manual_seed(21)
    x = torch.randn((B, Tn, Cc), generator=g0)
    scale = torch.randn((B, Tn, Cc), generator=g0)
    shift = -(scale * x)  # float32 product: fma(scale, x, shift) is the rounding error of the product, either sign or zero
    film = torch.cat([shift, scale], dim=2).contiguous()
    xd, fd = x.cuda(), film.cuda()
    img = torch.zeros((B, Tn, Cc), dtype=torch.bfloat16, device="cuda")
    _ok(lib.ma_wavegrad_pack_bf16(xd.data_ptr(), B, Tn, 1, Cc, Cc, 0, fd.data_ptr(), 2 * Cc, None, 0, 0.25, 1.0, img.data_ptr(), None, 0.0, None))
    dop = torch.ones((B, Tn, Cc), device="cuda")
    dfilm = torch.zeros((B, Tn, 2 * Cc), device="cuda")
    dx = torch.zeros((B, Tn, Cc), device="cuda")
    _ok(lib.ma_wavegrad_pack_bwd_f32(dop.data_ptr(), Cc, xd.data_ptr(), B, Tn, 1, Cc, fd.data_ptr(), 2 * Cc, 0.25, 1.0, None, 0.0, dx.data_ptr(), 0,
                                     dfilm.data_ptr(), 2 * Cc, 0, None))
    torch.cuda.synchronize()
    negative = torch.signbit(img.float().cpu()) & (img.float().cpu() != 0)
    assert int(negative.sum()) > 100 and int((~negative).sum()) > 100
    dshift = dfilm[:, :, :Cc].cpu()
    want = torch.where(negative, torch.tensor(0.25), torch.tensor(1.0)) * torch.tensor(1.0 / math.sqrt(2.0), dtype=torch.float64).float()
    assert torch.equal(dshift, want)


# ---- init convolution backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tn,C0,taps", [(3, 8, 3), (300, 32, 5), (257, 8, 7)])
def test_init_conv_bwd(torch, lib, Tn, C0, taps):
    """Integers: exact.  More than one workgroup per utterance at T = 300 and 257 (256 rows each)."""
    B = 2
    dout, audio = ints(torch, (B, Tn, C0), 31), ints(torch, (B, Tn), 32)
    parts = lib.ma_wavegrad_init_bwd_parts(B, Tn)
    stride = (taps + 1) * C0
    part, pw = guarded(torch, torch.zeros(parts * stride))
    dd, ad = dout.cuda(), audio.cuda()
    _ok(lib.ma_wavegrad_init_conv_bwd_f32(dd.data_ptr(), ad.data_ptr(), B, Tn, taps, C0, part.data_ptr(), None))
    dw, db = reduce_parts(torch, lib, part, stride, parts, [(0, taps * C0), (taps * C0, C0)])
    assert guard_intact(torch, pw, part.numel())
    half = taps // 2
    ap = torch.nn.functional.pad(audio.double(), (half, half))
    want = torch.stack([(dout.double() * ap[:, j:j + Tn, None]).sum(dim=(0, 1)) for j in range(taps)])
    assert torch.equal(dw.view(taps, C0).double(), want)
    assert torch.equal(db.double(), dout.double().sum(dim=(0, 1)))


# ---- the products ----------------------------------------------------------------------------------------------------------------------
def _image(torch, lib, x, halo, bf=True):
    """The operand image of x (B, T, C) through the forward's producer (slope 1, mul 1)."""
    B, Tn, Cc = x.shape
    cp = (Cc + 63) // 64 * 64 if bf else Cc
    xd = x.contiguous().cuda()
    img = torch.zeros((B, Tn + 2 * halo, cp), dtype=torch.bfloat16 if bf else torch.float32, device="cuda")
    if bf:
        _ok(lib.ma_wavegrad_pack_bf16(xd.data_ptr(), B, Tn, 1, Cc, cp, halo, None, 0, None, 0, 1.0, 1.0, img.data_ptr(), None, 0.0, None))
    else:
        _ok(lib.ma_wavegrad_pack_f32(xd.data_ptr(), B, Tn, 1, Cc, halo, None, 0, None, 0, 1.0, 1.0, img.data_ptr(), None, 0.0, None))
    torch.cuda.synchronize()
    return img


def _weights(torch, lib, w, mode, rows_fwd=None):
    """ma_wavegrad_weights_bf16 on one master w (N, taps, C) -> (fwd (rows_fwd, taps, Cpad), rev) bf16 on the device."""
    from mindaudio_amd import _lib
    from mindaudio_amd.train import plans

    n, k, c = w.shape
    cp, npad = (c + 63) // 64 * 64, (n + 63) // 64 * 64
    rows_fwd = n if rows_fwd is None else rows_fwd
    wd = w.contiguous().cuda()
    fwd = torch.full((rows_fwd * k * cp + 64,), float("nan"), dtype=torch.bfloat16, device="cuda")
    rev = torch.full(((k * cp if mode else c * k) * npad + 64,), float("nan"), dtype=torch.bfloat16, device="cuda")
    item = _lib.WaveGradWeightItem(wd.data_ptr(), fwd.data_ptr(), rev.data_ptr(), n, k, c, cp, npad, rows_fwd, mode, 0)
    table = plans.ItemTable([(item, (npad * k * cp + 255) // 256)], "cuda")
    _ok(lib.ma_wavegrad_weights_bf16(*table.args, None))
    torch.cuda.synchronize()
    assert bool(torch.isnan(fwd[-64:].float()).all()) and bool(torch.isnan(rev[-64:].float()).all())
    return fwd[:-64].view(rows_fwd, k, cp), rev[:-64]


@pytest.mark.parametrize("n,c,k,mode,rows_fwd", [(8, 8, 3, 0, 64), (128, 64, 3, 0, 128), (16, 8, 5, 1, 16), (64, 128, 2, 1, 64)])
def test_weight_copies(torch, lib, n, c, k, mode, rows_fwd):
    g0 = torch.Generator().manual_seed(n + c)
    w = torch.randn((n, k, c), generator=g0)
    fwd, rev = _weights(torch, lib, w, mode, rows_fwd)
    cp, npad = (c + 63) // 64 * 64, (n + 63) // 64 * 64
    want = torch.zeros((rows_fwd, k, cp))
    want[:n, :, :c] = w
    assert torch.equal(fwd.cpu(), want.to(torch.bfloat16))
    wb = torch.zeros((npad, k, cp))
    wb[:n, :, :c] = w
    wb = wb.to(torch.bfloat16)
    if mode:
        assert torch.equal(rev.view(k * cp, npad).cpu(), wb.permute(1, 2, 0).reshape(k * cp, npad))
    else:
        assert torch.equal(rev.view(c, k, npad).cpu(), wb[:, :, :c].flip(1).permute(2, 1, 0).contiguous())


def _tn_ws(torch, lib, mo, no, kc):
    nbytes = int(lib.ma_gemm_tn_workspace_bytes(mo, no, kc))
    return torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda"), nbytes


@pytest.mark.parametrize("bf", [True, False])
def test_dw_by_taps(torch, lib, bf):
    """B = 3, dilation 8 = the halo, N = 8 under Npad = 64.  The edge rows of utterances 0 and 2 hold large values and utterance 1's
    gradient is zero except at its first and last row: every cross-utterance term would show, and the result is exact on integers.
    The padded columns of the gradient image are overwritten with NaN after it is made: they are never read."""
    from mindaudio_amd.models import wavegrad_train as WT

    B, Tn, n, c, taps, d, h = 3, 20, 8, 16, 3, 8, 8
    dout, x = ints(torch, (B, Tn, n), 41), ints(torch, (B, Tn, c), 42)
    x[0, -8:], x[2, :8] = 64.0, -64.0
    dout[1, 1:-1] = 0
    gimg, ximg = _image(torch, lib, dout, h, bf), _image(torch, lib, x, h, bf)
    if bf:
        gimg[:, :, n:] = float("nan")
    gw, gww = guarded(torch, torch.zeros(n, taps, c))
    gb = torch.zeros(n, device="cuda")
    ws, nbytes = _tn_ws(torch, lib, n, c, B * (Tn + 2 * h))
    WT.conv_dw(lib, bf, gimg.data_ptr(), gimg.shape[2], ximg.data_ptr(), ximg.shape[2], gw.data_ptr(), gb.data_ptr(), n, c, taps, d,
               B * (Tn + 2 * h), ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    assert guard_intact(torch, gww, gw.numel())
    want = torch.nn.grad.conv1d_weight(x.double().transpose(1, 2), (n, c, taps), dout.double().transpose(1, 2), padding=d, dilation=d)
    assert torch.equal(gw.cpu().double(), want.permute(0, 2, 1))
    assert torch.equal(gb.cpu().double(), dout.double().sum(dim=(0, 1)))


@pytest.mark.parametrize("bf", [True, False])
@pytest.mark.parametrize("acc", [0, 1])
def test_dx_through_reversed_weights(torch, lib, bf, acc):
    """dX of a dilated 3-tap convolution on integers, exact; C = 8 real columns in rows of 64 floats (the rest untouched)."""
    from mindaudio_amd.models import wavegrad_train as WT

    B, Tn, n, c, taps, d, h = 2, 21, 16, 8, 3, 4, 8
    dout, w = ints(torch, (B, Tn, n), 51), ints(torch, (n, taps, c), 52)
    gimg = _image(torch, lib, dout, h, bf)
    ld = 64 if bf else c
    out0 = ints(torch, (B, Tn, ld), 53)
    out, outw = guarded(torch, out0)
    if bf:
        _, rev = _weights(torch, lib, w, 0)
        wp = rev.data_ptr()
    else:
        wd = w.contiguous().cuda()
        wp = wd.data_ptr()
    WT.conv_dx(lib, bf, gimg.data_ptr(), gimg.shape[2], wp, out.data_ptr(), ld, acc, B, Tn, h, n, c, taps, d, None)
    torch.cuda.synchronize()
    assert guard_intact(torch, outw, out.numel())
    want = torch.nn.grad.conv1d_input((B, c, Tn), w.double().permute(0, 2, 1), dout.double().transpose(1, 2), padding=d, dilation=d)
    want = want.transpose(1, 2) + (out0[:, :, :c].double() if acc else 0)
    assert torch.equal(out.cpu()[:, :, :c].double(), want)
    assert torch.equal(out.cpu()[:, :, c:], out0[:, :, c:])


@pytest.mark.parametrize("bf", [True, False])
@pytest.mark.parametrize("f,c", [(2, 64), (5, 8)])
def test_down_bwd(torch, lib, bf, f, c):
    """The kernel = stride = f convolution's backward on integers, exact: dX, dW added per utterance, db.  c = 8 takes the path with one
    product per kernel position (padded columns), c = 64 the one product per utterance."""
    from mindaudio_amd.models import wavegrad_train as WT

    B, Tn, n, h = 2, 7, 16, 8
    dout, x, w = ints(torch, (B, Tn, n), 61), ints(torch, (B, Tn * f, c), 62), ints(torch, (n, f, c), 63)
    gimg, ximg = _image(torch, lib, dout, 0, bf), _image(torch, lib, x, h, bf)
    cp = ximg.shape[2]
    out, outw = guarded(torch, torch.zeros(B, Tn * f, cp))
    gw0, gb0 = ints(torch, (n, f, c), 64), ints(torch, (n,), 65)
    gw, gb = gw0.cuda(), gb0.cuda()
    if bf:
        _, rev = _weights(torch, lib, w, 1)
        wp = rev.data_ptr()
    else:
        wd = w.contiguous().cuda()
        wp = wd.data_ptr()
    ws, nbytes = _tn_ws(torch, lib, n, f * c if c == cp else c, Tn)
    WT.down_bwd(lib, bf, gimg.data_ptr(), gimg.shape[2], ximg.data_ptr(), cp, h, wp, out.data_ptr(), 0, gw.data_ptr(), gb.data_ptr(), B, Tn, n,
                c, f, ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    assert guard_intact(torch, outw, out.numel())
    wt, dy, xx = w.double().permute(0, 2, 1), dout.double().transpose(1, 2), x.double().transpose(1, 2)
    want_dx = torch.nn.grad.conv1d_input((B, c, Tn * f), wt, dy, stride=f).transpose(1, 2)
    want_dw = torch.nn.grad.conv1d_weight(xx, (n, c, f), dy, stride=f).permute(0, 2, 1)
    assert torch.equal(out.cpu()[:, :, :c].double(), want_dx)
    assert torch.equal(gw.cpu().double(), gw0.double() + want_dw)
    assert torch.equal(gb.cpu().double(), gb0.double() + dout.double().sum(dim=(0, 1)))


# ---- norm + clipped Adam -----------------------------------------------------------------------------------------------------------------
def _clip_adam(torch, lib, p, g, m, v, scale, clip, lr_t):
    n = p.numel()
    parts = lib.ma_wavegrad_sumsq_parts(n)
    part = torch.zeros(parts, dtype=torch.float64, device="cuda")
    flag, norm = torch.full((4,), 7, dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda")
    _ok(lib.ma_wavegrad_sumsq_f64(g.data_ptr(), n, part.data_ptr(), None))
    _ok(lib.ma_wavegrad_clip_adam_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, part.data_ptr(), parts, scale, clip, lr_t,
                                      T.BETA1, T.BETA2, T.ADAM_EPS, flag.data_ptr(), norm.data_ptr(), None))
    torch.cuda.synchronize()
    return int(flag[0].item()), float(norm[0].item())


@pytest.mark.parametrize("gain,n", [(0.01, 1000), (30.0, 1000), (30.0, 3 * 4096 * 4 + 8)])
def test_clip_adam(torch, lib, gain, n):
    """Norm below (gain 0.01) and above (30) the clip, one and several partials.  The norm within n 2^-52 + 2^-24 relative (a float64
    sum in another order, stored as float32).  With g the unscaled, clipped gradient (three roundings: unscale, the float32 factor,
    the product), mag_m = b1 |m0| + (1 - b1) |g| and s = sqrt(v) + eps:
      m   two products and a sum on top of g's three: 6 u mag_m (absolute: b1 m0 and (1 - b1) g may cancel);
      v   all terms positive, g^2 carries 6 u, two products and a sum: 9 u v;
      p   lr_t (dm / s + |m| ds / s^2) with ds <= 6 u s (half of v's error, the root, the sum), then the product with the float32
          lr_t, the quotient and the subtraction: u (lr_t (6 mag_m + 6 |m|) / s + 4 |update| + |p|)."""
    scale, clip, lr, t = 4096.0, 1.0, 1e-2, 3
    g0 = torch.Generator().manual_seed(71)
    p0, g_ = torch.randn(n, generator=g0), torch.randn(n, generator=g0) * gain * scale / math.sqrt(n)
    m0, v0 = torch.randn(n, generator=g0) * 0.01, torch.rand(n, generator=g0) * 1e-4
    lr_t = lr * math.sqrt(1 - T.BETA2 ** t) / (1 - T.BETA1 ** t)
    p, g, m, v = p0.cuda(), g_.cuda(), m0.cuda(), v0.cuda()
    flag, norm = _clip_adam(torch, lib, p, g, m, v, scale, clip, lr_t)
    want_norm = float((g_.double() / scale).pow(2).sum().sqrt())
    assert flag == 0 and abs(norm - want_norm) <= (n * 2.0 ** -52 + 2 * U) * want_norm
    assert (want_norm < clip) == (gain < 1)
    P, M, V = {"w": p0.double().clone()}, {"w": m0.double().clone()}, {"w": v0.double().clone()}
    T.clip_adam_step(P, {"w": g_.double()}, M, V, t, lr, scale, clip)
    ge = g_.double() / scale * (clip / max(want_norm, clip))
    mag_m = T.BETA1 * m0.double().abs() + T.ONE_MINUS_BETA1 * ge.abs()
    s = V["w"].sqrt() + T.ADAM_EPS
    upd = (P["w"] - p0.double()).abs()
    assert float(((m.cpu().double() - M["w"]).abs() / (6 * U * mag_m)).max()) <= 1.0
    assert float(((v.cpu().double() - V["w"]).abs() / (9 * U * V["w"])).max()) <= 1.0
    bound = U * (lr_t * (6 * mag_m + 6 * M["w"].abs()) / s + 4 * upd + p0.double().abs())
    assert float(((p.cpu().double() - P["w"]).abs() / bound).max()) <= 1.0


def test_clip_adam_overflow(torch, lib):
    """An inf gradient: the flag is set, parameters and moments keep their bits."""
    n = 4096
    g0 = torch.Generator().manual_seed(72)
    p0, g_, m0, v0 = (torch.randn(n, generator=g0) for _ in range(4))
    g_[1234] = float("inf")
    p, g, m, v = p0.cuda(), g_.cuda(), m0.cuda(), v0.abs().cuda()
    flag, _ = _clip_adam(torch, lib, p, g, m, v, 4096.0, 1.0, 1e-3)
    assert flag == 1
    assert torch.equal(p.cpu(), p0) and torch.equal(m.cpu(), m0) and torch.equal(v.cpu(), v0.abs())
    g[1234] = 0.0
    flag, _ = _clip_adam(torch, lib, p, g, m, v, 4096.0, 1.0, 1e-3)
    assert flag == 0 and not torch.equal(p.cpu(), p0)  # the flag is rewritten by every call


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
LOSS_SCALE = 4096.0


def _trainer(name, operands, lr=1e-3):
    import torch

    from mindaudio_amd.models import WaveGrad, WaveGradTrainer

    c = T.case(name)
    model = WaveGrad(c["hps"])
    model.load_state_dict(c["state"])
    model.cuda()
    tr = WaveGradTrainer(model, lr, max_grad_norm=1.0, loss_scale=LOSS_SCALE, operands=operands)
    audio, level, noise, spec = c["batch"]
    return c, model, tr, (audio.cuda(), level, noise.cuda(), spec.cuda())


def test_forward_bits(torch):
    """The trainer's pred is WaveGrad.forward's, bit for bit (bf16 mode, SMALL)."""
    from mindaudio_amd.models import WaveGrad

    c, model, tr, batch = _trainer("small", "bf16")
    plain = WaveGrad(c["hps"])
    plain.load_state_dict(c["state"])
    plain.cuda()
    want = plain(batch[0], batch[1], batch[3])
    tr.loss_and_grads(*batch)
    got = tr._steps[c["shape"]].pred
    assert torch.equal(got, want)
    assert torch.equal(model(batch[0], batch[1], batch[3]), want)  # the bound model still runs, on views of the flat masters


@pytest.mark.parametrize("name", T.F32_CASES)
def test_chain_f32(torch, name):
    c, model, tr, batch = _trainer(name, "f32")
    la, ga, aa = T.reference(name, "a", LOSS_SCALE)
    lb, gb, ab = T.reference(name, "b", LOSS_SCALE)
    loss = tr.loss_and_grads(*batch)
    got = {k: v.cpu() for k, v in tr.gradients().items()}
    assert set(got) == set(ga) and all(got[k].shape == ga[k].shape for k in ga)
    print("%s: loss %.9f (a) %.9f (b) %.9f" % (name, loss, la, lb))
    assert abs(loss - la) <= T.MARGIN * abs(lb - la) + 1e-6
    dp = tr.activation_gradients()["pred"].cpu()
    gs = torch.tensor(LOSS_SCALE / dp.numel(), dtype=torch.float64).float()
    assert torch.equal(dp, torch.sign(aa["pred"]).float() * gs)  # sign * float32(scale / (B T)): exact, the guard keeps every sign
    bad = T.check_f32(got, ga, gb)
    G, A, Bf = T.by_cell(got), T.by_cell(ga), T.by_cell(gb)
    worst = max(T.relrms(G[k], A[k]) / max(T.relrms(Bf[k], A[k]), 1e-300) for k in A)
    print("%s: worst error / form (b)'s own error %.3f" % (name, worst))
    assert not bad, bad
    # the loss over 5 steps
    steps, lr = 5, 1e-3
    ta, tb = (T.trajectory(c["state"], c["hps"], c["batch"], form, steps, lr, LOSS_SCALE, 1.0) for form in ("a", "b"))
    for i in range(steps):
        value, overflow, scale = tr.step(*batch, lr=lr)
        allowed = T.MARGIN * abs(tb[i] - ta[i]) + 1e-6
        print("step %d: loss %.8f, (a) %.8f, (b) %.8f, allowed %.2e" % (i, value, ta[i], tb[i], allowed))
        assert not overflow and scale == LOSS_SCALE
        assert abs(value - ta[i]) <= allowed, (i, value, ta[i], allowed)


@pytest.mark.parametrize("name", T.BF16_CASES)
def test_chain_bf16(torch, name):
    """Per parameter group relrms(device, (a)) <= 2 S with S = relrms((c), (a)) <= 0.2, and the cosine over all parameters >= 0.98."""
    c, model, tr, batch = _trainer(name, "bf16")
    la, ga, _ = T.reference(name, "a", LOSS_SCALE)
    lc, gc, _ = T.reference(name, "c", LOSS_SCALE)
    loss = tr.loss_and_grads(*batch)
    got = {k: v.cpu() for k, v in tr.gradients().items()}
    bad, table, cos = T.check_bf16(got, ga, gc)
    print("%s: loss %.6f (a) %.6f (c) %.6f, cosine %.5f, (c)'s own %.5f" % (name, loss, la, lc, cos, T.cosine(gc, ga)))
    for k, (err, S) in sorted(table.items()):
        print("  %-22s device %.4f  S %.4f" % (k, err, S))
    assert not bad, bad
    assert cos >= T.COS_MIN
    print("%s: launches %s" % (name, tr.launches))


@pytest.mark.parametrize("operands", ["bf16", "f32"])
def test_same_bits_from_run_to_run(torch, operands):
    c, model, tr, batch = _trainer("tiny_b3", operands)
    l1 = tr.loss_and_grads(*batch)
    g1 = {k: v.clone() for k, v in tr.gradients().items()}
    l2 = tr.loss_and_grads(*batch)
    assert l1 == l2 and all(torch.equal(g1[k], v) for k, v in tr.gradients().items())
    c2, model2, tr2, _ = _trainer("tiny_b3", operands)
    assert tr2.loss_and_grads(*batch) == l1 and all(torch.equal(g1[k], v) for k, v in tr2.gradients().items())
    s1, s2 = tr.step(*batch), tr2.step(*batch)
    assert s1 == s2 and torch.equal(tr.params.master, tr2.params.master) and torch.equal(tr.params.moment2, tr2.params.moment2)


def test_utterances_do_not_see_each_other(torch):
    """Float32 operands.  Changing utterance 1's data leaves utterance 0's gradient at the last convolution's input bit-identical, and
    its pred and pred gradient too."""
    c, model, tr, batch = _trainer("tiny_b2", "f32")
    audio, level, noise, spec = batch
    tr.loss_and_grads(*batch)
    st = tr._steps[c["shape"]]
    last = st.ops[-1]
    n0 = st.T * last["C"] * 4

    def rows0():
        g = st.gws[st.goff[last["inp"]]:st.goff[last["inp"]] + n0].clone()
        return st.pred[0].clone(), tr.activation_gradients()["pred"][0].clone(), g

    before = rows0()
    first = {k: v.clone() for k, v in tr.gradients().items()}
    audio2, noise2, spec2 = audio.clone(), noise.clone(), spec.clone()
    audio2[1], spec2[1] = audio2[1] * -3.0 + 1.0, 1.0 - spec2[1]
    noise2[1] = -noise2[1]
    tr.loss_and_grads(audio2, level, noise2, spec2)
    after = rows0()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert any(not torch.equal(first[k], v) for k, v in tr.gradients().items())


def test_it_learns(torch):
    """30 steps on one TINY batch in bf16 mode lower the loss by at least half of what form (a)'s own 30 steps gain."""
    c, model, tr, batch = _trainer("tiny_b2", "bf16")
    steps, lr = 30, 1e-3
    ta = T.trajectory(c["state"], c["hps"], c["batch"], "a", steps, lr, LOSS_SCALE, 1.0)
    gain = ta[0] - ta[-1]
    assert gain > 0
    first = tr.step(*batch, lr=lr)[0]
    for _ in range(steps - 1):
        tr.step(*batch, lr=lr)
    last = tr.loss_and_grads(*batch)
    print("form (a): %.6f -> %.6f; device: %.6f -> %.6f" % (ta[0], ta[-1], first, last))
    assert first - last >= 0.5 * gain


def test_state_dict_round_trip(torch):
    """state_dict() names and shapes are the reference's; a second trainer loaded from it continues with the same bits."""
    c, model, tr, batch = _trainer("tiny_b2", "bf16")
    tr.step(*batch)
    sd = tr.state_dict()
    shapes = C.param_shapes(c["hps"])
    for k, shape in shapes.items():
        assert tuple(sd[k].shape) == tuple(shape) and tuple(sd["moment1." + k].shape) == tuple(shape) and "moment2." + k in sd
    assert int(sd["steps"]) == 1
    c2, model2, tr2, _ = _trainer("tiny_b2", "bf16")
    tr2.load_state_dict({k: v.cpu() for k, v in sd.items()})
    a, b = tr.step(*batch), tr2.step(*batch)
    assert a == b and torch.equal(tr.params.master, tr2.params.master)


def test_train_script_checkpoint_resume(torch, tmp_path):
    """Two steps of wavegrad.train on a manifest of 8 utterances, SaveCallBack's two files at step 2, a resume that continues at step 3
    from cur_step and the restored moments; the restored model gives WaveGrad.forward the trainer's bits."""
    import numpy as np

    import mindaudio_amd.wavegrad.train as script
    from mindaudio_amd.models import WaveGrad, WaveGradTrainer
    from mindaudio_amd.utils import ckpt
    from mindaudio_amd.wavegrad.config import Config
    from mindaudio_amd.wavegrad.dataset import FEATURE_POSTFIX, WAV_POSTFIX

    rng = np.random.RandomState(3)
    hop, crop, lines = T.TINY["hop_samples"], 4, []
    for i in range(8):
        wav = str(tmp_path / ("u%d.wav" % i))
        frames = 6 + i % 3
        np.save(wav.replace(".wav", WAV_POSTFIX), rng.uniform(-0.5, 0.5, size=frames * hop).astype(np.float32))
        np.save(wav.replace(".wav", FEATURE_POSTFIX), rng.uniform(0, 1, size=(T.TINY["n_mels"], frames)).astype(np.float32))
        lines.append("%s\t%s\n" % (wav, wav.replace(".wav", ".txt")))
    (tmp_path / "manifest.csv").write_text("".join(lines))
    hps = Config(dict(T.TINY, num_epochs=2, batch_size=2, learning_rate=1e-3, max_grad_norm=1.0, save_step=2, save_dir=str(tmp_path / "out"),
                      crop_mel_frames=crop, manifest_path=str(tmp_path / "manifest.csv"), data_path=str(tmp_path)))
    log = []
    losses = script.train(hps, log=log.append, max_steps=2)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and "step: 2," in log[1]
    model_path, opt_path = str(tmp_path / "out" / "model_2.ckpt"), str(tmp_path / "out" / "optimiser_2.ckpt")
    raw, opt = ckpt.read_mindspore_ckpt(model_path), ckpt.read_mindspore_ckpt(opt_path)
    assert int(raw["cur_step"]) == 2 and int(opt["cur_step"]) == 2 and int(opt["global_step"]) == 2
    assert raw["UBlock.0.block1.weight"].shape == (16, 16, 1, 1) and "moment1.last_conv.weight" in opt and "moment2.DBlock.0.bias" in opt
    # the restored model and a restored trainer agree bit for bit
    model = WaveGrad(hps)
    ckpt.load_mindspore_checkpoint(model, model_path)
    model.cuda()
    tr = WaveGradTrainer(WaveGrad(hps), 1e-3)
    assert script.restore(tr, model_path) == 2 and tr.steps == 2
    tr.model.cuda()
    c = T.case("tiny_b2")
    audio, level, noise, spec = c["batch"]
    batch = (audio.cuda(), level, noise.cuda(), spec.cuda())
    want = model(batch[0], batch[1], batch[3])
    tr.loss_and_grads(*batch)
    assert torch.equal(tr._steps[c["shape"]].pred, want)
    m1 = tr.state_dict()["moment1.last_conv.weight"]
    assert torch.equal(m1.cpu(), torch.from_numpy(opt["moment1.last_conv.weight"][:, :, 0, :])) and float(m1.abs().max()) > 0
    # the resumed run continues at step 3
    log2 = []
    more = script.train(hps, restore_path=model_path, log=log2.append, max_steps=1)
    assert len(more) == 1 and "step: 3," in log2[0]
