#!/usr/bin/env python3
"""Generate tests/golden/wavegrad_normalize.npz by running THE REFERENCE's `_normalize` (examples/wavegrad/preprocess.py:27-30) on
about 200 float32 values.

Runs only where the reference tree exists; nothing of it travels - preprocess.py is imported by path behind sys.modules stubs for
what it imports at the top and `_normalize` does not use (mindspore, mindspore.dataset.audio, dataset, ljspeech, config, tqdm,
mindaudio.data.io), and only the inputs and the results are stored.

  x (n,) float32 - 0, 1e-5, 1e-6, values around the clip at 1e-5, values above 1e5, and a log-uniform spread over 1e-7 .. 1e6
  y (n,) float32 - the reference's result
No figure is measured on the code under test.

usage: python tests/golden/gen_wavegrad_goldens.py <reference root>   (or MINDAUDIO_REFERENCE=<reference root>)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(root):
    def stub(name, **attrs):
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
        return mod

    ms = stub("mindspore")
    ms.dataset = stub("mindspore.dataset")
    ms.dataset.audio = stub("mindspore.dataset.audio", MelScale=None, Spectrogram=None)
    stub("dataset", FEATURE_POSTFIX="_feature.npy", WAV_POSTFIX="_wav.npy")
    stub("ljspeech", LJSpeech=None, create_ljspeech_tts_dataset=None)
    stub("config", load_config=None)
    stub("tqdm", tqdm=lambda it, **kw: it)
    ma = stub("mindaudio")
    ma.data = stub("mindaudio.data")
    ma.data.io = stub("mindaudio.data.io", read=None)
    spec = importlib.util.spec_from_file_location("reference_wavegrad_preprocess",
                                                  os.path.join(root, "examples", "wavegrad", "preprocess.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MINDAUDIO_REFERENCE")
    if not root or not os.path.isdir(root):
        sys.exit(__doc__.strip().splitlines()[-1])
    R = load_reference(root)
    rng = np.random.RandomState(20261)
    fixed = [0.0, 1e-5, 1e-6, 9.9e-6, 1.01e-5, 1.0, 10.0, 1e5, 1.5e5, 3e5, 1e6, 99999.0, 100001.0, 1e-4, 1e-3]
    spread = 10.0 ** rng.uniform(-7.0, 6.0, size=185)
    x = np.concatenate([np.asarray(fixed), spread]).astype(np.float32)
    y = R._normalize(x.copy())
    assert y.dtype == np.float32 and y.shape == x.shape
    path = os.path.join(HERE, "wavegrad_normalize.npz")
    np.savez(path, x=x, y=y)
    print(path, os.path.getsize(path), "bytes;", len(x), "values; clipped low", int((y == 0).sum()), "high", int((y == 1).sum()))


if __name__ == "__main__":
    main()
