"""CPU: the host halves of the phase-vocoder mirrors (data.augment.phase_vocoder_steps, spectrum._pad_shape, argument checks), the
C entry's argument checks (they return before any launch, so they run without a device), and the consistency of the fixtures that
tests/golden/gen_phase_vocoder_goldens.py recorded from the reference."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import phase_vocoder_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def specs():
    return np.load(C.SPECS)


@pytest.fixture(scope="module")
def fix():
    return np.load(C.GOLDENS)


@pytest.fixture(scope="module")
def wfix():
    return np.load(C.WAVE_GOLDENS)


@pytest.mark.parametrize("case", list(C.VOCODER_CASES))
def test_steps_equal_the_recorded_tables(specs, fix, case):
    from mindaudio_amd.data.augment import phase_vocoder_steps

    name, rate = C.VOCODER_CASES[case]
    index, alpha = phase_vocoder_steps(specs[name + "/spec"].shape[-1], rate)
    assert index.dtype == np.int32 and alpha.dtype == np.float64
    assert np.array_equal(index, fix[case + "/index"]) and np.array_equal(alpha, fix[case + "/alpha"])


@pytest.mark.parametrize("frames,rate", [(1251, 0.9), (7, 0.3), (10, 0.1), (33, 3.0)])
def test_steps_are_the_references_arange(frames, rate):
    from mindaudio_amd.data.augment import phase_vocoder_steps

    steps = np.arange(0, frames, rate, dtype=np.float64)  # augment.py:841
    index, alpha = phase_vocoder_steps(frames, rate)
    assert len(index) == len(alpha) == len(steps)
    assert index.tolist() == [int(s) for s in steps] and alpha.tolist() == [np.mod(s, 1.0) for s in steps]
    assert index.min() == 0 and index.max() <= frames - 1 and (alpha >= 0).all() and (alpha < 1).all()


def test_pad_shape():
    from mindaudio_amd.data.spectrum import _pad_shape

    y = np.arange(12, dtype=np.float64).reshape(2, 6)
    longer = _pad_shape(y, 9)
    assert longer.shape == (2, 9) and np.array_equal(longer[:, :6], y) and not longer[:, 6:].any() and longer.dtype == y.dtype
    assert np.array_equal(_pad_shape(y, 4), y[:, :4])
    assert _pad_shape(y, 6) is y
    assert np.array_equal(_pad_shape(np.arange(5.0), 7), [0, 1, 2, 3, 4, 0, 0])
    import torch

    t = torch.arange(12.0).reshape(2, 6)
    assert torch.equal(_pad_shape(t, 8), torch.nn.functional.pad(t, (0, 2))) and torch.equal(_pad_shape(t, 3), t[:, :3])
    assert _pad_shape(t, 6) is t


def test_mirrors_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mindaudio_amd._lib import MindaudioAmdError
    from mindaudio_amd.data import augment as A

    with pytest.raises(MindaudioAmdError):
        A.time_stretch(np.zeros(1024, np.float32), 0.9)
    with pytest.raises(MindaudioAmdError):
        A.pitch_shift(np.zeros((2, 1024), np.float32), 16000, 2)
    with pytest.raises(MindaudioAmdError):
        A._phase_vocoder(np.zeros((65, 9), np.complex64), 1.1)


def test_rate_is_checked_before_any_gpu_use():
    from mindaudio_amd.data import augment as A

    x = np.zeros(1024, np.float32)
    for rate in (0, 0.0, -1.5):
        with pytest.raises(ValueError, match="rate must be a positive number"):
            A.time_stretch(x, rate)
        with pytest.raises(ValueError, match="rate must be a positive number"):
            A._phase_vocoder(np.zeros((65, 9), np.complex64), rate)
    with pytest.raises(TypeError):
        A.time_stretch(x)  # the reference's rate=None default fails on `rate <= 0`
    assert {"time_stretch", "pitch_shift", "phase_vocoder_steps"} <= set(A.__all__)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """Without a device a launch would answer MA_ERR_LAUNCH: every bad argument is answered by its own code instead."""
    from mindaudio_amd import _build, _lib

    _build.build()
    lib = _lib.load()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)  # (never dereferenced: the checks return first)

    def call(spec=p, layout=_lib.STFT_FRAME_MAJOR, b=2, frames=9, n_freq=65, index=p, alpha=p, t_out=10, hop=32, out=p):
        return lib.ma_phase_vocoder_f32(spec, layout, b, frames, n_freq, index, alpha, t_out, hop, out, null)

    assert call(hop=0) == _lib.MA_ERR_HOP and call(hop=-3) == _lib.MA_ERR_HOP
    for bad in (dict(n_freq=1), dict(n_freq=0), dict(t_out=0), dict(frames=0), dict(b=0), dict(layout=2), dict(layout=-1),
                dict(spec=null), dict(index=null), dict(alpha=null), dict(out=null)):
        assert call(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    with pytest.raises(ValueError):
        _lib.check(call(hop=0), "_phase_vocoder")


def test_fixtures_are_complete_and_consistent(specs, fix, wfix):
    assert sorted(specs.files) == sorted(name + "/spec" for name in C.INPUTS)
    keys = ("out64", "out", "cols", "index", "alpha", "e_acc", "e32", "e_acc_all", "e32_all")
    assert sorted(fix.files) == sorted("%s/%s" % (case, k) for case in C.VOCODER_CASES for k in keys)
    for case, (name, rate) in C.VOCODER_CASES.items():
        (offsets, n, n_fft, hop), spec = C.INPUTS[name], specs[name + "/spec"]
        assert spec.dtype == np.complex64 and spec.shape == (len(offsets), n_fft // 2 + 1, 1 + n // hop)
        steps = len(fix[case + "/index"])
        if case in C.EXPECTED_STEPS:
            assert C.EXPECTED_STEPS[case] == (spec.shape[-1], steps)
        cols = fix[case + "/cols"]
        assert np.array_equal(cols, C.kept_steps(steps)) and cols[0] == 0 and cols[-1] == steps - 1
        out64, out = fix[case + "/out64"], fix[case + "/out"]
        assert out64.dtype == np.complex128 and out.dtype == np.complex64
        assert out64.shape == out.shape == spec.shape[:-1] + (len(cols),)
        assert fix[case + "/alpha"].shape == (steps,) and fix[case + "/index"].max() <= spec.shape[-1] - 1
        # step 0 is the first column itself (alpha 0, acc = its angle)
        assert np.abs(out64[..., 0] - spec[..., 0]).max() <= 4 * 2.0 ** -24 * np.abs(spec[..., 0]).max()
        assert np.allclose(fix[case + "/e_acc"], C.errors(out, out64), rtol=1e-12, atol=0)  # (taken over the kept steps)
        for e_acc, e32 in ((fix[case + "/e_acc"], fix[case + "/e32"]), (fix[case + "/e_acc_all"], fix[case + "/e32_all"])):
            assert e_acc.shape == e32.shape == (2,) and (e32 > 0).all()
            if steps > 8:  # a single-precision evaluation with a float64 accumulator is far better than the float32 accumulator
                assert (e32 < e_acc).all(), (case, e32, e_acc)
    keys = ("wave64", "wave", "cols", "length", "e_acc", "e32", "e_acc_all", "e32_all")
    assert sorted(wfix.files) == sorted("%s/%s" % (case, k) for case in C.WAVE_CASES for k in keys)
    for case, spec_ in C.WAVE_CASES.items():
        x, length = spec_["x"](), int(wfix[case + "/length"])
        if spec_["fn"] == "time_stretch":
            assert length == int(round(x.shape[-1] / spec_["args"][0]))
        else:  # pitch_shift keeps the STRETCHED length
            assert length == int(round(x.shape[-1] / 2.0 ** (-float(spec_["args"][1]) / 12)))
        if case in C.EXPECTED_SHAPES:
            assert x.shape[:-1] + (length,) == C.EXPECTED_SHAPES[case]
        cols = wfix[case + "/cols"]
        assert np.array_equal(cols, C.kept_samples(length))
        assert wfix[case + "/wave64"].shape == wfix[case + "/wave"].shape == x.shape[:-1] + (len(cols),)
        assert wfix[case + "/wave64"].dtype == wfix[case + "/wave"].dtype == np.float64
        assert np.allclose(wfix[case + "/e_acc"], C.errors(wfix[case + "/wave"], wfix[case + "/wave64"]), rtol=1e-12, atol=0)
        assert (wfix[case + "/e32"] < wfix[case + "/e_acc"]).all() and (wfix[case + "/e32_all"] < wfix[case + "/e_acc_all"]).all(), case
