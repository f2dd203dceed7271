"""GPU: data.augment._phase_vocoder / time_stretch / pitch_shift (csrc/phase_vocoder.hip between the stft, istft and resample kernels)
against the fixtures tests/golden/gen_phase_vocoder_goldens.py recorded from the reference's own functions.

Two references per case.  `out64` / `wave64` is the reference's formula evaluated with a float64 phase accumulator (its own code on a
complex128 spectrogram); the device, which accumulates in float64 too, is held to it by the project's margin on `e32`, the error of a
single-precision CPU evaluation: 8 x e32 in relative rms and 16 x e32 in max-abs over peak, each with a floor of 8 * 2^-24
(test_augment_gpu.py).  `out` / `wave` is what the reference returns for a complex64 spectrogram - a float32 accumulator that rounds a
growing phase at every step - and differs from `out64` by the recorded `e_acc`; the device is held to it by e_acc + the bound above
(triangle inequality).  The fixtures keep a subset of the steps / samples (phase_vocoder_cases.kept_steps, kept_samples) of every row
and bin, and e32 / e_acc are the generator's figures over that same subset; results of the two input layouts, of repeated runs and
of rows alone are compared in full, bit for bit.

Measured on an MI355X: the ERRTABLE in DESIGN.md 8.2.1."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import phase_vocoder_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def specs():
    return np.load(C.SPECS)


@pytest.fixture(scope="module")
def fix():
    return np.load(C.GOLDENS)


@pytest.fixture(scope="module")
def wfix():
    return np.load(C.WAVE_GOLDENS)


def _check(tag, y, ref64, ref, e32, e_acc):
    rms, mx = C.errors(y, ref64)
    rms_ref, mx_ref = C.errors(y, ref.astype(ref64.dtype), scale=ref64)  # (on e_acc's scale: the triangle inequality is exact)
    b_rms, b_mx = max(8 * e32[0], FLOOR), max(16 * e32[1], FLOOR)
    print("ERRTABLE %s e32 %.3g %.3g e_acc %.3g %.3g gpu_vs_f64 %.3g %.3g gpu_vs_reference %.3g %.3g" % (
        tag, e32[0], e32[1], e_acc[0], e_acc[1], rms, mx, rms_ref, mx_ref))
    assert rms <= b_rms, (rms, b_rms)
    assert mx <= b_mx, (mx, b_mx)
    assert rms_ref <= e_acc[0] + b_rms, (rms_ref, e_acc[0], b_rms)
    assert mx_ref <= e_acc[1] + b_mx, (mx_ref, e_acc[1], b_mx)


def _frame_major_view(torch, spec):
    """(B, n_freq, frames) as spectrum.stft returns it: a transposed view of (B, frames, n_freq) memory."""
    v = torch.from_numpy(spec).cuda().transpose(1, 2).contiguous().transpose(1, 2)
    assert not v.is_contiguous() or v.shape[1] == 1 or v.shape[2] == 1
    return v


@pytest.mark.parametrize("case", list(C.VOCODER_CASES))
def test_vocoder_against_the_reference(torch, specs, fix, case):
    from mindaudio_amd.data import augment as A

    name, rate = C.VOCODER_CASES[case]
    spec, hop = specs[name + "/spec"], C.INPUTS[name][3]
    cols = fix[case + "/cols"]
    results = {"frame_major": A._phase_vocoder(_frame_major_view(torch, spec), rate),
               "bin_major": A._phase_vocoder(torch.from_numpy(spec).cuda(), rate, hop_length=hop)}
    for layout, y in results.items():
        assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.complex64 and y.is_contiguous()
        assert tuple(y.shape) == spec.shape[:-1] + (len(fix[case + "/index"]),)
        _check("%s %s" % (case, layout), y.cpu().numpy()[..., cols], fix[case + "/out64"], fix[case + "/out"], fix[case + "/e32"],
               fix[case + "/e_acc"])
    assert torch.equal(torch.view_as_real(results["frame_major"]), torch.view_as_real(results["bin_major"]))
    y_np = A._phase_vocoder(spec, rate)  # NumPy in -> NumPy out, the same bits
    assert isinstance(y_np, np.ndarray) and y_np.dtype == np.complex64
    assert np.array_equal(y_np.view(np.float32), results["bin_major"].cpu().numpy().view(np.float32))


@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("case", list(C.WAVE_CASES))
def test_waveform_against_the_reference(torch, wfix, case, as_tensor):
    from mindaudio_amd.data import augment as A

    spec_ = C.WAVE_CASES[case]
    x = spec_["x"]()
    y = getattr(A, spec_["fn"])(torch.from_numpy(x).cuda() if as_tensor else x, *spec_["args"])
    if as_tensor:
        assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32
        y = y.cpu().numpy()
    else:
        assert isinstance(y, np.ndarray) and y.dtype == np.float64
    assert y.shape == x.shape[:-1] + (int(wfix[case + "/length"]),)
    if case in C.EXPECTED_SHAPES:
        assert y.shape == C.EXPECTED_SHAPES[case]
    _check("%s %s" % (case, "tensor" if as_tensor else "numpy"), y[..., wfix[case + "/cols"]], wfix[case + "/wave64"],
           wfix[case + "/wave"], wfix[case + "/e32"], wfix[case + "/e_acc"])


def test_two_runs_and_rows_alone_give_the_same_bits(torch, specs):
    from mindaudio_amd.data import augment as A

    for name, rate in (("w4000", 1.25), ("w1250", 0.8), ("w3000", 0.9)):
        spec = specs[name + "/spec"]
        assert spec.shape[0] == 2
        for dev in (_frame_major_view(torch, spec), torch.from_numpy(spec).cuda()):
            first = torch.view_as_real(A._phase_vocoder(dev, rate)).clone()
            assert torch.equal(torch.view_as_real(A._phase_vocoder(dev, rate)), first)
            for b in range(2):
                alone = A._phase_vocoder(dev[b:b + 1], rate)
                assert torch.equal(torch.view_as_real(alone)[0], first[b])
                assert torch.equal(torch.view_as_real(A._phase_vocoder(dev[b], rate)), first[b])  # (n_freq, frames), no batch axis
    x = torch.from_numpy(C.WAVE_CASES["pitch_up4"]["x"]()).cuda()
    for fn, args in ((A.time_stretch, (0.8,)), (A.pitch_shift, (16000, 4))):
        first = fn(x, *args).clone()
        assert torch.equal(fn(x, *args), first)
        for b in range(2):
            assert torch.equal(fn(x[b:b + 1], *args)[0], first[b]) and torch.equal(fn(x[b], *args), first[b])


def test_time_stretch_is_the_composition_of_its_pieces(torch):
    """No hidden copy path with other arithmetic: stft's frame-major memory goes into the vocoder as it is."""
    from mindaudio_amd.data import augment as A
    from mindaudio_amd.data import spectrum as S

    x = torch.from_numpy(C.WAVE_CASES["stretch_0.8"]["x"]()).cuda()
    for rate in (0.8, 1.25):
        spec = S.stft(x)
        assert not spec.is_contiguous() and spec.transpose(1, 2).is_contiguous()
        stretched = A._phase_vocoder(spec, rate)
        want = S.istft(stretched, length=int(round(x.shape[-1] / rate)))
        assert torch.equal(A.time_stretch(x, rate), want)
        # and the copy path gives the same spectrogram
        assert torch.equal(torch.view_as_real(A._phase_vocoder(spec.contiguous(), rate)), torch.view_as_real(stretched))


def test_entry_point_rejects_bad_arguments(torch):
    from mindaudio_amd import _lib

    lib = _lib.load()
    spec = torch.zeros((2, 9, 65, 2), device="cuda")
    index = torch.zeros(10, dtype=torch.int32, device="cuda")
    alpha = torch.zeros(10, dtype=torch.float64, device="cuda")
    out = torch.full((2, 65, 10, 2), 7.0, device="cuda")
    P, null = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(0)

    def call(spec=P(spec), layout=_lib.STFT_FRAME_MAJOR, b=2, frames=9, n_freq=65, index=P(index), alpha=P(alpha), t_out=10, hop=32,
             out=P(out)):
        return lib.ma_phase_vocoder_f32(spec, layout, b, frames, n_freq, index, alpha, t_out, hop, out, null)

    assert call(hop=0) == _lib.MA_ERR_HOP
    for bad in (dict(n_freq=1), dict(t_out=0), dict(frames=0), dict(b=0), dict(layout=2), dict(spec=null), dict(index=null),
                dict(alpha=null), dict(out=null)):
        assert call(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    assert call() == _lib.MA_OK  # an all-zero spectrogram: magnitude 0 everywhere
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
