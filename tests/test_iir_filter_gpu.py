"""GPU: data.filters.cal_filter_by_coffs / low_pass_filter / peaking_equalizer / filtfilt (csrc/iir_filter.hip) against the fixtures
tests/golden/gen_iir_goldens.py recorded from the reference's own functions.  Every sample of every case is compared.

Float32 results (the biquads on float32 input; filtfilt on a float32 tensor, against the reference run on the float32-rounded
input) are held to the project's standing margins on e_in, the reference's sensitivity to one single-precision rounding of its
input: 8 x e_in in relative rms and 16 x e_in in max-abs over peak, each with a floor of 8 * 2^-24 (test_phase_vocoder_gpu.py,
test_augment_gpu.py).  Float64 results are held to 16 x max(e_re, 2^-44) in both figures, e_re being the recorded spread between
float64 evaluation orders: the device's chunk length and its fused multiply-adds are one more order.  Results of repeated runs, of
rows alone, of NumPy and tensor input and of the reverse pass are compared bit for bit.

Measured on an MI355X: the ERRTABLE in DESIGN.md 8.2.2."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import iir_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -24
FLOOR64 = 2.0 ** -44


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def fix():
    return np.load(C.GOLDENS)


def _check32(tag, y, ref, e_in):
    rms, mx = C.errors(y, ref)
    print("ERRTABLE %s f32 e_in %.3g %.3g gpu %.3g %.3g" % (tag, e_in[0], e_in[1], rms, mx))
    assert rms <= max(8 * e_in[0], FLOOR), (rms, e_in)
    assert mx <= max(16 * e_in[1], FLOOR), (mx, e_in)


def _check64(tag, y, ref, e_re):
    rms, mx = C.errors(y, ref)
    print("ERRTABLE %s f64 e_re %.3g %.3g gpu %.3g %.3g" % (tag, e_re[0], e_re[1], rms, mx))
    assert rms <= 16 * max(e_re[0], FLOOR64), (rms, e_re)
    assert mx <= 16 * max(e_re[1], FLOOR64), (mx, e_re)


@pytest.mark.parametrize("case", list(C.BIQUAD_CASES))
def test_biquads_against_the_reference(torch, fix, case):
    from mindaudio_amd.data import filters as F

    fn, args, shape, _ = C.BIQUAD_CASES[case]
    x, ref = fix[case + "/x"], fix[case + "/out"]
    keep = x.copy()
    y = getattr(F, fn)(x, *args)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == shape
    assert np.array_equal(x, keep) and not np.shares_memory(x, y)  # the one departure: the input is left alone
    _check32(case, y, ref, fix[case + "/e_in"])
    xt = torch.from_numpy(x).cuda()
    yt = getattr(F, fn)(xt, *args)
    assert isinstance(yt, torch.Tensor) and yt.is_cuda and yt.dtype == torch.float32 and tuple(yt.shape) == shape
    assert np.array_equal(yt.cpu().numpy().view(np.uint32), y.view(np.uint32))  # NumPy in and tensor in: the same bits
    assert torch.equal(xt.cpu(), torch.from_numpy(keep))
    # float64 in -> float64 out, against the reference's float64 result on the same values
    y64 = getattr(F, fn)(x.astype(np.float64), *args)
    assert y64.dtype == np.float64
    _check64(case, y64, fix[case + "/out64"], fix[case + "/e_re"])
    assert np.array_equal(y64.astype(np.float32).view(np.uint32), y.view(np.uint32))  # one recursion, two output roundings
    if len(shape) == 2 and shape[1] > 1:  # a channel alone: the same bits as inside the batch
        for ch in range(shape[1]):
            alone = getattr(F, fn)(np.ascontiguousarray(x[:, ch]), *args)
            assert np.array_equal(alone.view(np.uint32), y[:, ch].view(np.uint32))
            assert np.array_equal(getattr(F, fn)(np.ascontiguousarray(x[:, ch:ch + 1]), *args).view(np.uint32),
                                  y[:, ch:ch + 1].view(np.uint32))


@pytest.mark.parametrize("case", list(C.FILTFILT_CASES))
def test_filtfilt_against_the_reference(torch, fix, case):
    from mindaudio_amd.data import filters as F

    args, shape = C.FILTFILT_CASES[case]
    x, ref, ref32, e_in, e_re = (fix[case + "/" + k] for k in ("x", "out", "out32", "e_in", "e_re"))
    y = F.filtfilt(x, *args)
    assert isinstance(y, np.ndarray) and y.dtype == np.float64 and y.shape == shape
    _check64(case + " numpy", y, ref, e_re)
    yt = F.filtfilt(torch.from_numpy(x).cuda(), *args)
    assert isinstance(yt, torch.Tensor) and yt.is_cuda and yt.dtype == torch.float64 and tuple(yt.shape) == shape
    assert np.array_equal(yt.cpu().numpy().view(np.uint64), y.view(np.uint64))
    assert np.array_equal(F.filtfilt(x, *args).view(np.uint64), y.view(np.uint64))  # two runs
    x32 = x.astype(np.float32)
    y32 = F.filtfilt(torch.from_numpy(x32).cuda(), *args)
    assert y32.is_cuda and y32.dtype == torch.float32 and tuple(y32.shape) == shape
    _check32(case + " tensor32", y32.cpu().numpy(), ref32, e_in)
    y32n = F.filtfilt(x32, *args)  # float32 NumPy in: float64 out, as SciPy's
    assert y32n.dtype == np.float64
    _check64(case + " numpy32", y32n, ref32, e_re)
    rows = x.reshape(-1, shape[-1])
    if rows.shape[0] > 1:  # a row alone
        flat = y.reshape(rows.shape)
        for r in range(rows.shape[0]):
            assert np.array_equal(F.filtfilt(rows[r], *args).view(np.uint64), flat[r].view(np.uint64))
            assert np.array_equal(F.filtfilt(rows[r:r + 1], *args).view(np.uint64), flat[r:r + 1].view(np.uint64))
    # the chunk-carried plan and a forced sequential one are two evaluation orders of one filter
    y_seq = F.filtfilt(x, *args, _sequential=True)
    _check64(case + " sequential", y_seq, ref, e_re)
    _check64(case + " carry-vs-sequential", y, y_seq, e_re)


def test_the_clamp_is_upper_only_and_outside_the_recursion(torch, fix):
    from mindaudio_amd.data import filters as F

    case = C.CLAMP_CASE
    fn, args, shape, _ = C.BIQUAD_CASES[case]
    x, ref, unclamped = fix[case + "/x"], fix[case + "/out"], fix[case + "/unclamped"]
    y = getattr(F, fn)(x, *args)
    assert y.max() == 1.0 and (y == 1.0).sum() >= 1 and y.min() < -1.0  # nothing above 1, some exactly 1, below -1 passes
    clamped = np.flatnonzero(unclamped > 1.0 + 1e-6)
    assert len(clamped) > 10 and np.all(y[clamped] == 1.0)
    after = np.unique(np.concatenate([clamped + k for k in (1, 2, 3)]))
    after = after[(after < len(y)) & (unclamped[np.minimum(after, len(y) - 1)] < 1.0 - 1e-6)]
    assert len(after) > 10
    # had the recursion gone on from the clamped value, the next samples would be off by a1 * (y - 1): far above this
    assert np.abs(y[after].astype(np.float64) - unclamped[after]).max() <= 2.0 ** -22
    assert np.abs(y[after] - ref[after]).max() <= 2.0 ** -22


def test_reverse_rows_alone_and_repeated_runs_give_the_same_bits(torch, fix):
    from mindaudio_amd.data import filters as F

    b, a, zi, padlen = F.filtfilt_design(4, 0.1, "lowpass")
    for dtype in (torch.float32, torch.float64):
        for T in (1, 3, C.L - 1, C.L, C.L + 1, 3 * C.L + 7, C.LONG):
            x = torch.from_numpy(C.noise(T, (3, T))).cuda().to(dtype)
            for kw in (dict(), dict(zi=zi, zi_mode="times-x0"), dict(zi=zi, zi_mode="as-is"), dict(upper_clamp=True)):
                fwd = F.iir_filter_device(x, b, a, **kw)
                assert torch.equal(F.iir_filter_device(x, b, a, **kw), fwd)
                for r in range(3):
                    assert torch.equal(F.iir_filter_device(x[r:r + 1].contiguous(), b, a, **kw)[0], fwd[r])
                rev = F.iir_filter_device(x.flip(1).contiguous(), b, a, reverse=True, **kw)
                assert torch.equal(rev.flip(1), fwd)  # the reverse pass = the forward pass on the flipped row, flipped back
                inplace = x.clone()
                assert F.iir_filter_device(inplace, b, a, out=inplace, **kw) is inplace and torch.equal(inplace, fwd)
            if T > C.L:  # several chunks against one per row
                seq = F.iir_filter_device(x, b, a, zi=zi, zi_mode="times-x0", plan=F.iir_plan(b, a, T, sequential=True))
                e = C.errors(F.iir_filter_device(x, b, a, zi=zi, zi_mode="times-x0").cpu().numpy(), seq.cpu().numpy())
                assert max(e) <= (16 * FLOOR64 if dtype == torch.float64 else 2.0 ** -22), (T, e)


def test_filtfilt_is_the_composition_of_its_pieces(torch, fix):
    from mindaudio_amd.data import filters as F

    for case in ("lp4_2d", "bp8", "hp8_seq"):
        args, shape = C.FILTFILT_CASES[case]
        b, a, zi, padlen = F.filtfilt_design(*args)
        x = torch.from_numpy(fix[case + "/x"]).cuda()
        ext = F.odd_extend(x, padlen)
        assert np.array_equal(ext.cpu().numpy(), C.odd_ext(fix[case + "/x"], padlen))
        fwd = F.iir_filter_device(ext, b, a, zi, "times-x0")
        bwd = F.iir_filter_device(fwd, b, a, zi, "times-x0", reverse=True)
        assert torch.equal(F.filtfilt(x, *args), bwd[:, padlen:-padlen])
        # and the backward pass is the forward pass on the flipped signal
        assert torch.equal(F.iir_filter_device(fwd.flip(1).contiguous(), b, a, zi, "times-x0").flip(1), bwd)


def test_entry_point_rejects_bad_arguments(torch):
    from mindaudio_amd import _lib

    lib = _lib.load()
    x = torch.zeros((2, 1000), device="cuda")
    out = torch.full((2, 1000), 7.0, device="cuda")
    ws = torch.zeros(1 << 12, dtype=torch.float64, device="cuda")
    b, a, zi = np.array([0.5, 0.2, 0.1]), np.array([1.0, -0.3, 0.2]), np.array([0.1, 0.2])
    big = np.zeros(18)
    big[0] = 1.0
    power = np.linalg.matrix_power(C.transition(a), 256)
    H, P, null = (lambda arr: arr.ctypes.data_as(ctypes.c_void_p)), (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(0)

    def call(x=P(x), y=P(out), sample_bytes=4, rows=2, T=1000, order=2, chunk=256, b=H(b), a=H(a), zi=H(zi), zi_mode=2,
             power=H(power), filt=True, ws=P(ws), ws_bytes=ws.numel() * 8, steps=0):
        f = _lib.IirFilter(order, zi_mode, 0, 1, chunk, b, a, zi, power, steps, 0)
        return lib.ma_iir_filter(x, sample_bytes, rows, T, ctypes.byref(f) if filt else None, y, ws, ws_bytes, null)

    for bad in (dict(x=null), dict(y=null), dict(filt=False), dict(b=null), dict(a=null), dict(power=null), dict(rows=0), dict(T=0),
                dict(order=0), dict(chunk=0), dict(sample_bytes=2), dict(zi_mode=3), dict(steps=8), dict(a=H(np.array([2.0, -0.3, 0.2])))):
        assert call(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    assert call(order=17, b=H(big), a=H(big)) == _lib.MA_ERR_UNSUPPORTED
    assert call(ws=null) == _lib.MA_ERR_WORKSPACE and call(ws_bytes=8) == _lib.MA_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    assert call() == _lib.MA_OK  # an all-zero input: zi * 0, all-zero output
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
