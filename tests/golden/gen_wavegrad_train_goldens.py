#!/usr/bin/env python3
"""Generate tests/golden/wavegrad_train_goldens.npz by running THE REFERENCE's `diffuse` and `batch_collate`
(examples/wavegrad/dataset.py:10-18, 53-85) under a fixed np.random seed.

Runs only where the reference tree exists; nothing of it travels - dataset.py is imported by path behind sys.modules stubs for what
it imports at the top (ljspeech), `batch_collate` (a closure of create_wavegrad_dataset) is caught from the `per_batch_map` argument
of a stand-in dataset object, and only the inputs and the results are stored.

  S, start, end, hop, crop       the schedule and the crop geometry (scalars)
  noise_level (S + 1,) float32   what create_wavegrad_dataset computed (read back from the closure's hps / recomputed identically)
  x (n,) float32, seed_diffuse   diffuse's input;  d_noisy, d_scale, d_noise its three results under np.random.seed(seed_diffuse)
  audio_<i>, spec_<i>, seed_batch   three utterances (the last shorter than its crop: zero padding);  b_noisy, b_scale, b_noise, b_spec
No figure is measured on the code under test.

usage: python tests/golden/gen_wavegrad_train_goldens.py <reference root>   (or MINDAUDIO_REFERENCE=<reference root>)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
S, START, END, HOP, CROP, N_MELS = 60, 1e-4, 0.05, 12, 4, 8


class _Pipeline:
    """Stands in for the MindSpore dataset: remembers the per-batch map."""

    caught = None

    def map(self, **kw):
        return self

    def batch(self, batch_size, per_batch_map=None, **kw):
        _Pipeline.caught = per_batch_map
        return self


def load_reference(root):
    mod = types.ModuleType("ljspeech")
    mod.LJSpeech = lambda **kw: None
    mod.create_ljspeech_tts_dataset = lambda ds, **kw: _Pipeline()
    sys.modules["ljspeech"] = mod
    spec = importlib.util.spec_from_file_location("reference_wavegrad_dataset", os.path.join(root, "examples", "wavegrad", "dataset.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MINDAUDIO_REFERENCE")
    if not root or not os.path.isdir(root):
        sys.exit(__doc__.strip().splitlines()[-1])
    R = load_reference(root)
    hps = types.SimpleNamespace(data_path="", manifest_path="", noise_schedule_start=START, noise_schedule_end=END, noise_schedule_S=S,
                                hop_samples=HOP, crop_mel_frames=CROP)
    R.create_wavegrad_dataset(hps, 3)
    collate = _Pipeline.caught
    beta = hps.noise_schedule
    noise_level = np.concatenate([[1.0], np.cumprod(1 - beta) ** 0.5], axis=0).astype(np.float32)
    rng = np.random.RandomState(20262)
    out = dict(S=S, start=START, end=END, hop=HOP, crop=CROP, noise_level=noise_level, seed_diffuse=11, seed_batch=12)
    x = rng.uniform(-1, 1, size=50).astype(np.float32)
    np.random.seed(11)
    out["x"] = x
    out["d_noisy"], out["d_scale"], out["d_noise"] = R.diffuse(x, S, noise_level)
    audio, spec = [], []
    for i, (frames, n) in enumerate(((7, 7 * HOP), (9, 9 * HOP + 5), (6, 3 * HOP + 3))):
        audio.append(rng.uniform(-1, 1, size=n).astype(np.float32))
        spec.append(rng.uniform(0, 1, size=(N_MELS, frames)).astype(np.float32))
        out["audio_%d" % i], out["spec_%d" % i] = audio[-1], spec[-1]
    np.random.seed(12)
    out["b_noisy"], out["b_scale"], out["b_noise"], out["b_spec"] = collate(audio, spec)
    path = os.path.join(HERE, "wavegrad_train_goldens.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes; batch", out["b_noisy"].shape, out["b_scale"], "zero tail", int((out["b_noisy"][2] == out["b_noise"][2] * (1 - out["b_scale"][2] ** 2) ** 0.5).sum()))


if __name__ == "__main__":
    main()
