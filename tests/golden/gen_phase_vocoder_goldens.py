#!/usr/bin/env python3
"""Generate the phase-vocoder fixtures by running THE REFERENCE's stft, _phase_vocoder, istft, resample, time_stretch and pitch_shift
(mindaudio/data/{spectrum,processing,augment}.py) in the build container on the cases of tests/phase_vocoder_cases.py.

Runs only where the reference tree exists; nothing of it travels - its modules are imported by path behind the `mindspore` stub of
gen_goldens.py, as gen_augment_goldens.py does, and only spectrograms, results and error figures are stored.  The reference's istft
needs np.float_ (removed in NumPy 2): the alias is restored for the duration of the run, as in gen_goldens.istft_goldens.

Vocoder cases (phase_vocoder_specs.npz, phase_vocoder_goldens.npz):
  <input>/spec   the reference's complex64 stft of the input
  <case>/out64   the reference's _phase_vocoder on spec.astype(complex128): its own formula with a float64 accumulator (complex128)
  <case>/out     the reference's _phase_vocoder on spec itself: float32 accumulator (complex64)
  <case>/index, <case>/alpha   the step tables; <case>/cols the kept steps of out64 / out
  <case>/e_acc   [relative rms, max-abs over peak] of out against out64: what the float32 accumulator costs
  <case>/e32     the same figures for a SINGLE-PRECISION CPU evaluation (float32 angle, magnitude, mix, sine and cosine; float64
                 accumulator reduced modulo 2 pi) against out64: the yardstick of test_phase_vocoder_gpu.py
                 Both over the KEPT steps, the population the tests compare (the phase error grows with the step, and the kept steps
                 hold the last four of every case); <case>/e_acc_all, <case>/e32_all: over the whole result, DESIGN.md's table.
Waveform cases (time_stretch_goldens.npz): wave = the reference function itself, wave64 = the same reference functions with the
spectrogram cast to complex128 before the vocoder, e_acc, and e32 from the whole chain in single precision (scipy.fft keeps float32),
over the kept samples and (_all) over the whole result.  No figure is measured on the code under test.

usage: python tests/golden/gen_phase_vocoder_goldens.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy.fft as sfft
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import phase_vocoder_cases as C  # noqa: E402

F = np.float32
TWO_PI = 2.0 * np.pi


def load_reference():
    spec = importlib.util.spec_from_file_location("gen_goldens", os.path.join(HERE, "gen_goldens.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    gg._install_stubs()
    for name in ("mindaudio", "mindaudio.data"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    return {m: gg._load("mindaudio.data." + m, "mindaudio/data/%s.py" % m) for m in ("io", "spectrum", "filters", "processing", "augment")}


# ---- single-precision evaluations of the reference's formulas ------------------------------------------------------------------------
def vocoder32(spec, index, alpha, hop):
    assert spec.dtype == np.complex64
    phi = np.linspace(0, np.pi * hop, spec.shape[-2])
    pad = np.pad(spec, [(0, 0)] * (spec.ndim - 1) + [(0, 2)])
    ang, mag = np.angle(pad), np.abs(pad)
    assert ang.dtype == F and mag.dtype == F
    acc = ang[..., 0].astype(np.float64)
    out = np.zeros(spec.shape[:-1] + (len(index),), np.complex64)
    for t, (i, a) in enumerate(zip(index, alpha)):
        m = (F(1) - F(a)) * mag[..., i] + F(a) * mag[..., i + 1]
        r = (acc - TWO_PI * np.round(acc / TWO_PI)).astype(F)
        re, im = m * np.cos(r), m * np.sin(r)
        assert re.dtype == F and im.dtype == F
        out[..., t].real, out[..., t].imag = re, im
        d = ang[..., i + 1].astype(np.float64) - ang[..., i].astype(np.float64) - phi
        acc += phi + (d - TWO_PI * np.round(d / TWO_PI))
    return out


def stft32(x, n_fft=512):
    hop = n_fft // 4
    win = scipy.signal.get_window("hann", n_fft, fftbins=True).astype(F)
    xp = np.pad(x.astype(F), [(0, 0)] * (x.ndim - 1) + [(n_fft // 2, n_fft // 2)])
    frames = 1 + (xp.shape[-1] - n_fft) // hop
    fr = np.stack([xp[..., t * hop:t * hop + n_fft] * win for t in range(frames)], axis=-1)  # (..., n_fft, frames)
    spec = sfft.rfft(fr, axis=-2)
    assert spec.dtype == np.complex64
    return spec


def istft32(spec, length):
    n_fft = 2 * (spec.shape[-2] - 1)
    hop = n_fft // 4
    win = scipy.signal.get_window("hann", n_fft, fftbins=True).astype(F)
    n_frames = min(spec.shape[-1], int(np.ceil((length + n_fft) / hop)))
    y = np.zeros(spec.shape[:-2] + (n_fft + hop * (n_frames - 1),), F)
    wsum = np.zeros(y.shape[-1], F)
    fr = sfft.irfft(spec[..., :n_frames], n=n_fft, axis=-2)
    assert fr.dtype == F
    for t in range(n_frames):
        y[..., t * hop:t * hop + n_fft] += fr[..., t] * win
        wsum[t * hop:t * hop + n_fft] += win * win
    nz = wsum > 1e-9
    y[..., nz] /= wsum[nz]
    y = y[..., n_fft // 2:]
    if y.shape[-1] >= length:
        return y[..., :length]
    return np.pad(y, [(0, 0)] * (y.ndim - 1) + [(0, length - y.shape[-1])])


def time_stretch32(x, rate):
    from mindaudio_amd.data.augment import phase_vocoder_steps  # host only: np.arange, checked against the reference's below

    spec = stft32(x)
    index, alpha = phase_vocoder_steps(spec.shape[-1], rate)
    return istft32(vocoder32(spec, index, alpha, 128), int(round(x.shape[-1] / rate)))


def pitch_shift32(x, sr, n_steps):
    rate = 2.0 ** (-float(n_steps) / 12)
    y = time_stretch32(x, rate)
    n = y.shape[-1]
    z = scipy.signal.resample(y, int(np.ceil(n * (float(sr) / (float(sr) / rate)))), axis=-1).astype(F)
    if z.shape[-1] >= n:
        return z[..., :n]
    return np.pad(z, [(0, 0)] * (z.ndim - 1) + [(0, n - z.shape[-1])])


def main():
    ref = load_reference()
    R, S, P = ref["augment"], ref["spectrum"], ref["processing"]
    from mindaudio_amd.data.augment import phase_vocoder_steps

    had = hasattr(np, "float_")
    if not had:
        np.float_ = np.float64
    try:
        specs, out = {}, {}
        for name in C.INPUTS:
            x, n_fft, hop = C.vocoder_input(name)
            specs[name] = np.ascontiguousarray(S.stft(x, n_fft=n_fft, hop_length=hop))
            assert specs[name].dtype == np.complex64
        for case, (name, rate) in C.VOCODER_CASES.items():
            spec, hop = specs[name], C.INPUTS[name][3]
            out64 = R._phase_vocoder(spec.astype(np.complex128), rate)
            ref32 = R._phase_vocoder(spec, rate)
            assert out64.dtype == np.complex128 and ref32.dtype == np.complex64 and out64.shape == ref32.shape
            index, alpha = phase_vocoder_steps(spec.shape[-1], rate)
            assert len(index) == out64.shape[-1] and index.dtype == np.int32
            if case in C.EXPECTED_STEPS:
                assert C.EXPECTED_STEPS[case] == (spec.shape[-1], len(index)), (case, spec.shape, len(index))
            cols = C.kept_steps(len(index))
            y32 = vocoder32(spec, index, alpha, hop)
            e_acc, e32 = C.errors(ref32[..., cols], out64[..., cols]), C.errors(y32[..., cols], out64[..., cols])
            out[case + "/e_acc_all"], out[case + "/e32_all"] = np.array(C.errors(ref32, out64)), np.array(C.errors(y32, out64))
            out[case + "/out64"], out[case + "/out"], out[case + "/cols"] = out64[..., cols], ref32[..., cols], cols
            out[case + "/index"], out[case + "/alpha"] = index, alpha
            out[case + "/e_acc"], out[case + "/e32"] = np.array(e_acc), np.array(e32)
            ea, e3 = out[case + "/e_acc_all"], out[case + "/e32_all"]
            print("%-14s %-16s -> %4d steps  whole: e_acc %.2g / %.2g  e32 %.2g / %.2g  ratio %.0f / %.0f   kept: e_acc %.2g / %.2g"
                  "  e32 %.2g / %.2g" % (case, spec.shape, len(index), ea[0], ea[1], e3[0], e3[1], ea[0] / e3[0], ea[1] / e3[1],
                                         e_acc[0], e_acc[1], e32[0], e32[1]))

        waves = {}
        for case, spec_ in C.WAVE_CASES.items():
            x = spec_["x"]()
            if spec_["fn"] == "time_stretch":
                rate, sr = spec_["args"][0], None
                wave = R.time_stretch(x, rate)
            else:
                sr, n_steps = spec_["args"]
                rate = 2.0 ** (-float(n_steps) / 12)
                wave = R.pitch_shift(x, sr, n_steps)
            # the same reference functions, the spectrogram cast to complex128 before the vocoder
            wave64 = S.istft(R._phase_vocoder(S.stft(x).astype(np.complex128), rate), length=int(round(x.shape[-1] / rate)))
            if sr is not None:
                wave64 = S._pad_shape(P.resample(wave64, orig_freq=float(sr) / rate, new_freq=sr), data_shape=wave64.shape[-1])
            y32 = time_stretch32(x, rate) if sr is None else pitch_shift32(x, sr, spec_["args"][1])
            assert wave.dtype == np.float64 and wave64.dtype == np.float64 and y32.dtype == F, (wave.dtype, wave64.dtype, y32.dtype)
            assert wave.shape == wave64.shape == y32.shape, (case, wave.shape, wave64.shape, y32.shape)
            if case in C.EXPECTED_SHAPES:
                assert wave.shape == C.EXPECTED_SHAPES[case], wave.shape
            cols = C.kept_samples(wave.shape[-1])
            e_acc, e32 = C.errors(wave[..., cols], wave64[..., cols]), C.errors(y32[..., cols], wave64[..., cols])  # (kept samples)
            waves[case + "/e_acc_all"], waves[case + "/e32_all"] = np.array(C.errors(wave, wave64)), np.array(C.errors(y32, wave64))
            waves[case + "/wave64"], waves[case + "/wave"], waves[case + "/cols"] = wave64[..., cols], wave[..., cols], cols
            waves[case + "/length"] = np.int64(wave.shape[-1])
            waves[case + "/e_acc"], waves[case + "/e32"] = np.array(e_acc), np.array(e32)
            print("%-14s %-14s -> %-14s e_acc %.2g / %.2g  e32 %.2g / %.2g" % (case, x.shape, wave.shape, e_acc[0], e_acc[1], e32[0],
                                                                             e32[1]))
    finally:
        if not had:
            del np.float_
    for path, arrays in ((C.SPECS, {k + "/spec": v for k, v in specs.items()}), (C.GOLDENS, out), (C.WAVE_GOLDENS, waves)):
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
