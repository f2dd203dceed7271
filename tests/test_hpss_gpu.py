"""GPU: data.features soft_mask / hpss / harmonic and median_filter_device (csrc/hpss.hip) against the fixtures
tests/golden/gen_hpss_goldens.py recorded from the reference's own functions.

Median filter, and hpss on real input with power 1 or 2.  Bit for bit: the two medians (the reference's scipy.ndimage results,
which the generator recorded inside its hpss), the masks and the masked spectrograms.  A median is a selection, and the mask
arithmetic is a handful of correctly rounded IEEE operations in the reference's order with no contraction, so nothing may differ;
a result that is merely close is a failure.  The same holds between a contiguous tensor, the frame-major transposed view that
stft returns, NumPy input and a repeated run.
soft_mask with power 0.5 or 3.7.  |mask - reference| <= 4 eps(dtype) absolute: the reference's and the device's pow are each within
2 ulp, so the two powers differ from the reference's by at most 3 eps relative; d(a / (a + b)) carries the factor m (1 - m) <= 1/4,
which gives 1.5 eps, and the add and the divide at most 1.5 eps more.  Powers 1, 2 and inf: bit for bit.
hpss on complex64 input.  The device's magnitudes may differ from np.abs by an ulp, so a selected median moves by an ulp: the
masked spectrograms within 8 * 2^-24 * |S| element by element, the masks within 4 * 2^-23.  The generator asserted that every
fixture magnitude is exactly zero or at least 1e-6, so no element sits at the `tiny` switch.
stft with n_fft = 2048 (the framing launch and the power-of-two FFT that harmonic goes through; the fused stft kernels stop at
1024).  The yardstick of test_features_gpu.py: |delta| <= 2e-6 x the frame's largest magnitude, against the float64 evaluation
oracle.speech_features.stft_vec, for the four padding modes, an odd hop, a short window, no centring and a batch.
harmonic.  The yardstick of test_augment_gpu.py: within 8 x e32 in relative rms and 16 x e32 in max-abs over peak, each with the floor
8 * 2^-24; e32 is the reference's harmonic as it stands against the same code with the spectrogram kept complex128, measured by
the generator.  A row inside a batch equals the row alone bit for bit.
Derived or recorded from the reference, never measured on the code under test.

Measured on an MI355X: the ERRTABLE in DESIGN.md 8.2.4."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hpss_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def fix():
    return np.load(C.GOLDENS)


def _frame_major(xt):
    """The same values as a (..., F, T) view of (..., T, F) memory: what stft returns."""
    v = xt.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not v.is_contiguous() or v.shape[-1] == 1 or v.shape[-2] == 1
    return v


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("case", list(C.REAL_CASES))
def test_medians_and_real_hpss_equal_the_reference(torch, fix, case):
    from mindaudio_amd.data import features as F

    c = C.REAL_CASES[case]
    x = C.real_input(case)
    assert C.sha(x) == str(fix["real/%s/sha" % case])
    keep = x.copy()
    xt = torch.from_numpy(x).cuda()
    xv = _frame_major(xt)
    pos = C.kept(x.shape)
    # the two median filters, in both memory orders and both types, against the reference's own scipy results
    seen = set()
    for kernel in c["kernels"]:
        for key, k, axis in zip(C.median_keys(case, kernel), C.pair(kernel), (-1, -2)):
            if key in seen:
                continue
            seen.add(key)
            ref = C.decode(x, fix[key], k, axis)
            for inp in (xt, xv):
                got = F.median_filter_device(inp, k, axis=axis)
                assert got.stride() == inp.stride() and got.data_ptr() != inp.data_ptr()
                assert _same(got.cpu().numpy(), ref), (key, inp.stride())
                got64 = F.median_filter_device(inp.double(), k, axis=axis)
                assert _same(got64.cpu().numpy(), ref.astype(np.float64)), (key, "float64", inp.stride())
    # masks and masked spectrograms
    for n_run, (kernel, power, margin) in enumerate(C.real_runs(case)):
        key = C.run_key(case, kernel, power, margin)
        kw = dict(kernel_size=kernel, power=power, margin=margin)
        mask_h, mask_p = F.hpss(xt, mask=True, **kw)
        out_h, out_p = F.hpss(xt, mask=False, **kw)
        got = {}
        for label, a in (("mask_h", mask_h), ("mask_p", mask_p), ("out_h", out_h), ("out_p", out_p)):
            assert isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == x.shape
            got[label] = a.cpu().numpy()
            ref = fix["%s/%s" % (key, label)]
            bad = int((got[label].reshape(-1)[pos] != ref).sum())
            print("ERRTABLE real %s %s: %d of %d differ" % (key, label, bad, len(ref)))
            assert _same(got[label].reshape(-1)[pos], ref), (key, label, bad)
        assert np.array_equal(got["out_h"], x * got["mask_h"]) and np.array_equal(got["out_p"], x * got["mask_p"])
        # the frame-major view, NumPy input and a second run give the same bits
        others = [F.hpss(xv, mask=False, **kw), F.hpss(xt, mask=False, **kw)]
        if n_run == 0:
            others.append(F.hpss(x, mask=False, **kw))
            assert all(isinstance(a, np.ndarray) for a in others[-1])
            others.append(F.hpss(xv, mask=True, **kw))
        for pair in others[:3]:
            for a, ref in zip(pair, (got["out_h"], got["out_p"])):
                assert _same(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, ref), key
        if n_run == 0:
            for a, ref in zip(others[3], (got["mask_h"], got["mask_p"])):
                assert _same(a.cpu().numpy(), ref), key
    assert np.array_equal(x, keep) and np.array_equal(xt.cpu().numpy(), keep) and np.array_equal(xv.cpu().numpy(), keep)


def test_other_real_types(torch):
    """float64 keeps its type (the medians are the same selections, the masks float64); anything else computes in float32."""
    from mindaudio_amd.data import features as F

    x = C.real_input("mid")
    m32 = F.hpss(x, mask=True)
    m64 = F.hpss(x.astype(np.float64), mask=True)
    for a, b in zip(m32, m64):
        assert a.dtype == np.float32 and b.dtype == np.float64
        # six float32 roundings of 2^-24 relative each (two quotients, two squares that double the quotients' share, the sum,
        # the last quotient) on a value of at most 1
        assert np.abs(a - b).max() <= FLOOR
    xi = np.round(x * 1000).astype(np.int16)
    for a, b in zip(F.hpss(xi, kernel_size=(17, 5)), F.hpss(xi.astype(np.float32), kernel_size=(17, 5))):
        assert _same(a, b)


@pytest.mark.parametrize("split_zeros", [False, True])
@pytest.mark.parametrize("power", C.POWERS, ids=["p%g" % p for p in C.POWERS])
@pytest.mark.parametrize("dtype", C.SOFT_DTYPES)
def test_soft_mask_against_the_reference(torch, fix, dtype, power, split_zeros):
    from mindaudio_amd.data import features as F

    a, b = fix["soft/%s/a" % dtype], fix["soft/%s/b" % dtype]
    keep_a, keep_b = a.copy(), b.copy()
    ref = fix[C.soft_key(dtype, power, split_zeros)]
    got = F.soft_mask(a, b, power=power, split_zeros=split_zeros)
    assert isinstance(got, np.ndarray) and got.dtype == ref.dtype and got.shape == ref.shape
    gt = F.soft_mask(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), power=power, split_zeros=split_zeros)
    assert isinstance(gt, torch.Tensor) and gt.is_cuda and _same(gt.cpu().numpy(), got)
    assert np.array_equal(a, keep_a) and np.array_equal(b, keep_b)
    if power in C.EXACT_POWERS:
        print("ERRTABLE soft %s p%g s%d: %d of %d differ" % (dtype, power, split_zeros, int((got != ref).sum()), ref.size))
        assert np.array_equal(got, ref)
        return
    bound = 4 * float(np.finfo(dtype).eps)
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print("ERRTABLE soft %s p%g s%d: bound %.3g gpu %.3g" % (dtype, power, split_zeros, bound, err))
    assert err <= bound, (err, bound)


def test_soft_mask_shapes_and_other_types(torch):
    from mindaudio_amd.data import features as F

    a = np.arange(24, dtype=np.int32).reshape(2, 3, 4)
    b = a[::-1].copy()
    got = F.soft_mask(a, b, power=2)
    ref = F.soft_mask(a.astype(np.float32), b.astype(np.float32), power=2)
    assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, ref)
    va, vb = np.float32([4.0, 0.0, 1.0, 1.0]), np.float32([4.0, 0.0, 1.0, 0.0])
    assert np.array_equal(F.soft_mask(va, vb, power=1, split_zeros=True), np.float32([0.5, 0.5, 0.5, 1.0]))
    assert np.array_equal(F.soft_mask(va, vb, power=3.7), np.float32([0.5, 0.0, 0.5, 1.0]))
    assert np.array_equal(F.soft_mask(va, vb, power=np.inf), [False, False, False, True])
    at = torch.from_numpy(a.astype(np.float32)).cuda()
    sliced = F.soft_mask(at[:, :, ::2], at.flip(0)[:, :, ::2], power=2)  # non-contiguous tensors
    assert np.array_equal(sliced.cpu().numpy(), ref[:, :, ::2])


@pytest.mark.parametrize("margin", C.COMPLEX_MARGINS, ids=["m%s" % C.tag(m) for m in C.COMPLEX_MARGINS])
def test_hpss_on_complex_input(torch, fix, margin):
    from mindaudio_amd.data import features as F

    xs = [C.complex_input(name) for name in C.COMPLEX_SLICES]
    for name, x in zip(C.COMPLEX_SLICES, xs):
        assert C.sha(x) == str(fix["complex/%s/sha" % name])
    pos = C.kept(C.COMPLEX_SHAPE)
    batch = np.stack(xs)
    results = {}
    for tag, inp in (("2d", xs[0]), ("batch", batch), ("batch_tensor", torch.from_numpy(batch).cuda())):
        masks = F.hpss(inp, mask=True, margin=margin)
        outs = F.hpss(inp, mask=False, margin=margin)
        if tag == "batch_tensor":
            assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in masks + outs)
            masks, outs = [a.cpu().numpy() for a in masks], [a.cpu().numpy() for a in outs]
        for m, o in zip(masks, outs):
            assert m.dtype == np.float32 and o.dtype == np.complex64 and m.shape == o.shape == inp.shape
        results[tag] = masks + outs
    for a, b in zip(results["batch"], results["batch_tensor"]):
        assert np.array_equal(a, b)
    for a, b in zip(results["2d"], results["batch"]):
        assert np.array_equal(a, b[0])  # a slice alone and inside the batch: the same bits
    for s, name in enumerate(C.COMPLEX_SLICES):
        mag = np.abs(xs[s]).reshape(-1)[pos].astype(np.float64)
        for label, a in zip(("mask_h", "mask_p", "out_h", "out_p"), results["batch"]):
            ref = fix["%s/%s" % (C.complex_key(name, margin), label)]
            err = np.abs(a[s].reshape(-1)[pos].astype(np.complex128) - ref.astype(np.complex128))
            if label.startswith("mask"):
                print("ERRTABLE complex %s m%s %s: bound %.3g gpu %.3g" % (name, C.tag(margin), label, 4 * 2.0 ** -23, err.max()))
                assert err.max() <= 4 * 2.0 ** -23, (name, label, err.max())
            else:
                worst = float((err / np.where(mag > 0, mag, 1.0)).max())
                print("ERRTABLE complex %s m%s %s: bound %.3g x |S| gpu %.3g x |S|" % (name, C.tag(margin), label, FLOOR, worst))
                assert np.all(err <= FLOOR * mag), (name, label, worst)


TOL_STFT = 2e-6  # test_features_gpu.py's: relative to the per-frame max magnitude


@pytest.mark.parametrize("kw", [dict(), dict(pad_mode="reflect", hop_length=300), dict(pad_mode="edge", win_length=1500),
                                dict(pad_mode="symmetric", window="hamming"), dict(center=False, hop_length=777),
                                dict(n_fft=4096, hop_length=1024)],
                         ids=["default", "reflect_hop300", "edge_win1500", "symmetric_hamming", "nocenter_hop777", "nfft4096"])
def test_stft_2048_vs_oracle(torch, kw):
    from oracle import speech_features as O

    from mindaudio_amd.data import spectrum as S

    kw = dict(dict(n_fft=2048), **kw)
    x = np.stack([C.harmonic_input("stft_row%d" % r) for r in range(3)])[:, :5000 + 123 * len(kw)]
    want = O.stft_vec(x, **kw)
    got = S.stft(x, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.complex64 and got.shape == want.shape
    scale = np.maximum(np.abs(want).max(axis=-2, keepdims=True), 1e-30)
    err = float((np.abs(got - want) / scale).max())
    print("ERRTABLE stft %s: bound %.3g gpu %.3g" % (kw, TOL_STFT, err))
    assert err <= TOL_STFT, err
    one = S.stft(x[1], **kw)  # a row alone: the reference's Fortran order for a 1-D wave, and the same bits
    assert one.flags["F_CONTIGUOUS"] and np.array_equal(one, got[1])
    gt = S.stft(torch.from_numpy(x).cuda(), **kw)
    assert gt.is_cuda and np.array_equal(gt.cpu().numpy(), got)
    ri = S.stft(x[:1], return_complex=False, **kw)
    assert ri.shape == want[:1].shape + (2,) and np.array_equal(ri[..., 0], got[:1].real) and np.array_equal(ri[..., 1], got[:1].imag)


def test_harmonic_against_the_reference_and_row_alone_equals_row_in_batch(torch, fix):
    from mindaudio_amd.data import features as F

    y = fix["harmonic/x"]
    keep = y.copy()
    ref, e32 = fix["harmonic/out"], fix["harmonic/e32"]
    got = F.harmonic(y)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == y.shape
    gt = F.harmonic(torch.from_numpy(y).cuda())
    assert isinstance(gt, torch.Tensor) and gt.is_cuda and gt.dtype == torch.float32 and tuple(gt.shape) == y.shape
    assert np.array_equal(gt.cpu().numpy().astype(np.float64), got)
    rms, mx = C.errors(got, ref)
    print("ERRTABLE harmonic e32 %.3g %.3g gpu %.3g %.3g" % (e32[0], e32[1], rms, mx))
    assert rms <= max(8 * e32[0], FLOOR), (rms, e32[0])
    assert mx <= max(16 * e32[1], FLOOR), (mx, e32[1])
    batch = np.stack([C.harmonic_input("harmonic_row0"), y, C.harmonic_input("harmonic_row2")])
    gb = F.harmonic(batch)
    assert gb.shape == batch.shape and gb.dtype == np.float64 and np.array_equal(gb[1], got)
    assert not np.array_equal(gb[0], gb[1])
    wide = F.harmonic(y, margin=3.0, kernel_size=(31, 17))  # the keyword arguments reach hpss
    assert wide.shape == y.shape and not np.array_equal(wide, got)
    assert np.array_equal(y, keep)


def test_errors_that_read_data_or_take_tensors(torch):
    from mindaudio_amd.data import features as F

    x = C.real_input("b3")
    xt = torch.from_numpy(x).cuda()
    neg = x.copy()
    neg[1, 4, :] = -1e-3  # (a whole row: the reference looks at the medians, and a single value never is one)
    for a, b in ((neg, x), (x, neg), (torch.from_numpy(neg).cuda(), xt)):
        with pytest.raises(TypeError, match="must be non-negative"):
            F.soft_mask(a, b)
    for inp in (neg, torch.from_numpy(neg).cuda()):
        with pytest.raises(TypeError, match="must be non-negative"):
            F.hpss(inp, kernel_size=5)
    with pytest.raises(TypeError, match="shape mismatch"):
        F.soft_mask(xt, xt[:, :, :5])
    with pytest.raises(TypeError, match="strictly positive"):
        F.soft_mask(xt, xt, power=0)
    with pytest.raises(TypeError, match="Margins must be >= 1.0"):
        F.hpss(xt, margin=(1.0, 0.5))
    for kernel in (49, (31, 37), 128):  # k > 4 n on the time axis (12), on the frequency axis (9), k > 127
        with pytest.raises(ValueError, match=r"<= 127 and size <= 4 \* axis length"):
            F.hpss(xt, kernel_size=kernel)
    with pytest.raises(ValueError, match=r"<= 127 and size <= 4 \* axis length"):
        F.median_filter_device(xt, 37, axis=-2)
    with pytest.raises(ValueError):
        F.median_filter_device(xt, 3, axis=0)
    with pytest.raises(ValueError):  # n_fft = 2048 does not fit
        F.harmonic(np.zeros(1000, np.float32))
