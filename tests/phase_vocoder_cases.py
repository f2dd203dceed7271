"""The cases of the phase-vocoder fixtures, shared by tests/golden/gen_phase_vocoder_goldens.py (which runs the reference's functions
on them) and test_phase_vocoder_cpu.py / test_phase_vocoder_gpu.py (which run ours).  Inputs are seeded recipes: segments of
tests/golden/BAC009S0002W0122.wav as float32, so the fixtures hold spectrograms, results and error figures only.

Three files, each below the size limit for a committed file:
  golden/phase_vocoder_specs.npz    <input>/spec: the reference's complex64 stft of every vocoder input (the rates of one input share it)
  golden/phase_vocoder_goldens.npz  per vocoder case out64, out, cols, index, alpha, e_acc, e32, e_acc_all, e32_all
  golden/time_stretch_goldens.npz   per waveform case wave64, wave, cols, length, e_acc, e32, e_acc_all, e32_all
`cols` are the kept steps / samples of the last axis (kept_steps / kept_samples below), of every row and bin: what the tests
compare, and what e_acc / e32 are taken over (the `_all` figures: over the whole result).
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WAV = os.path.join(HERE, "golden", "BAC009S0002W0122.wav")
SPECS = os.path.join(HERE, "golden", "phase_vocoder_specs.npz")
GOLDENS = os.path.join(HERE, "golden", "phase_vocoder_goldens.npz")
WAVE_GOLDENS = os.path.join(HERE, "golden", "time_stretch_goldens.npz")
_cache = {}


def wav():
    if "wav" not in _cache:
        from mindaudio_amd.data.io import read

        w, sr = read(WAV)
        assert sr == 16000 and w.shape == (95984,)
        _cache["wav"] = np.asarray(w, np.float64)
    return _cache["wav"]


def rows(offsets, n):
    """(len(offsets), n) float32: segments of the wav (speech: voiced stretches, consonants and near-silence)."""
    return np.stack([wav()[o:o + n] for o in offsets]).astype(np.float32)


# ---- vocoder cases: name -> (input, rate); input -> (offsets, n, n_fft, hop) ----------------------------------------------------------
INPUTS = {
    "w150": ((21000, 40000), 150, 128, 32),      # 5 frames
    "w1250": ((20000, 52000), 1250, 128, 32),    # 40 frames, 65 bins: one full tile of 64 and a one-bin tail
    "w9600": ((30000,), 9600, 128, 32),          # 301 frames
    "w4000": ((25000, 60000), 4000, 512, 128),   # 257 bins
    "w3000": ((15000, 45000), 3000, 400, 100),   # 201 bins
    "w4096": ((35000,), 4096, 2048, 512),        # 1025 bins
}
VOCODER_CASES = {
    "w150_r2": ("w150", 2.0),                    # 5 -> 3 steps: fewer steps than chunks; integer steps
    "w1250_r0.8": ("w1250", 0.8),                # 40 -> 50
    "w1250_r1": ("w1250", 1.0),
    "w1250_r2": ("w1250", 2.0),
    "w1250_r0.5": ("w1250", 0.5),
    "w1250_up4": ("w1250", 2.0 ** (4.0 / 12)),
    "w1250_down3": ("w1250", 2.0 ** (-3.0 / 12)),
    "w9600_r1.1": ("w9600", 1.1),                # 301 -> 274: many steps per chunk, ragged last chunk
    "w4000_r1.25": ("w4000", 1.25),
    "w3000_r0.9": ("w3000", 0.9),
    "w4096_r0.9": ("w4096", 0.9),
}
EXPECTED_STEPS = {"w150_r2": (5, 3), "w1250_r0.8": (40, 50), "w9600_r1.1": (301, 274)}  # frames -> steps, as the issue lists them


def vocoder_input(name):
    offsets, n, n_fft, hop = INPUTS[name]
    return rows(offsets, n), n_fft, hop


# ---- waveform cases ---------------------------------------------------------------------------------------------------------------------
def _w4000():
    return rows((25000, 60000), 4000)


WAVE_CASES = {
    "stretch_0.8": dict(fn="time_stretch", x=_w4000, args=(0.8,)),
    "stretch_1.25": dict(fn="time_stretch", x=_w4000, args=(1.25,)),
    "stretch_1d_0.5": dict(fn="time_stretch", x=lambda: rows((33000,), 2100)[0], args=(0.5,)),
    "stretch_3d_0.7": dict(fn="time_stretch", x=lambda: rows((12000, 28000, 47000, 70000), 3000).reshape(2, 2, 3000), args=(0.7,)),
    "pitch_up4": dict(fn="pitch_shift", x=_w4000, args=(16000, 4)),
    "pitch_down3": dict(fn="pitch_shift", x=_w4000, args=(16000, -3)),
    "pitch_1d_up2.5": dict(fn="pitch_shift", x=lambda: rows((25000,), 4000)[0], args=(16000, 2.5)),
}
EXPECTED_SHAPES = {"pitch_up4": (2, 5040)}  # the reference's length quirk, as the issue states it


# ---- which columns of a long last axis the fixtures keep ------------------------------------------------------------------------------
def kept_steps(steps):
    """The first and last four steps and every seventh in between (7 and the kernel's 8-step tiles share no factor)."""
    return np.array([t for t in range(steps) if t < 4 or t >= steps - 4 or t % 7 == 2], np.int64)


def kept_samples(n):
    """Both ends and every fifth sample."""
    return np.array([i for i in range(n) if i < 32 or i >= n - 32 or i % 5 == 2], np.int64)


def errors(y, ref, scale=None):
    """(relative rms, max-abs over peak) of y against ref, both relative to `scale` (default: ref itself)."""
    scale = ref if scale is None else scale
    err = np.abs(np.asarray(y).astype(scale.dtype) - ref)
    return float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(np.abs(scale) ** 2))), float(err.max() / np.abs(scale).max())
