#!/usr/bin/env python3
"""Generate the harmonic / percussive separation fixtures by running THE REFERENCE's soft_mask, hpss and harmonic
(mindaudio/data/features.py, with stft, istft and magphase of mindaudio/data/spectrum.py and scipy.ndimage.median_filter) in the
build container on the cases of tests/hpss_cases.py.

Runs only where the reference tree exists; nothing of it travels - its modules are imported by path behind the `mindspore` stub of
gen_goldens.py, as gen_processing_goldens.py does, and only inputs, results and error figures are stored
(tests/golden/hpss_goldens.npz; the layout is described in hpss_cases.py).

The two median filters: the reference's own intermediate arrays are taken by wrapping the median_filter its features module calls.
The generator asserts, on the reference alone, what the tests rely on: that both equal the brute-force periodic-reflection median
of hpss_cases.py (the window convention), that the offset encoding gives them back bit for bit, that the masks of the mixtures
take values across (0, 1), that every complex fixture magnitude is exactly zero or at least MAG_FLOOR, that the reference's
a ** 2.0 is a * a bit for bit, and that inputs are left as they were.
harmonic: e32 is the difference between the reference's harmonic as it stands (its stft rounds the spectrogram to complex64) and the
same code with the spectrogram kept complex128 (the spectrum module's NumPy handle replaced by one whose complex64 is complex128).
The reference needs np.float_ (removed in NumPy 2): the alias is restored for the duration of the run, as in gen_goldens.py.
No figure is measured on the code under test.

usage: python tests/golden/gen_hpss_goldens.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import hpss_cases as C  # noqa: E402


def load_reference():
    spec = importlib.util.spec_from_file_location("gen_goldens", os.path.join(HERE, "gen_goldens.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    gg._install_stubs()
    for name in ("mindaudio", "mindaudio.data"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    S = gg._load("mindaudio.data.spectrum", "mindaudio/data/spectrum.py")
    return gg._load("mindaudio.data.features", "mindaudio/data/features.py"), S


class Recorder:
    """Wraps the median_filter the reference's features module calls and keeps what came out, in call order."""

    def __init__(self, module):
        self.module, self.inner, self.out = module, module.median_filter, []

    def __enter__(self):
        self.module.median_filter = self
        return self

    def __exit__(self, *exc):
        self.module.median_filter = self.inner
        return False

    def __call__(self, x, size, mode):
        y = self.inner(x, size=size, mode=mode)
        self.out.append((tuple(size), np.array(y)))
        return y


class Complex128:
    """A stand-in for the spectrum module's `np`: everything is NumPy's, except that complex64 is complex128."""

    complex64 = np.complex128

    def __getattr__(self, name):
        return getattr(np, name)


def main():
    R, S = load_reference()
    out = {}

    # ---- real spectrograms: medians, masks, masked spectrograms ----
    for name, c in C.REAL_CASES.items():
        x = C.real_input(name)
        assert x.dtype == np.float32 and x.shape == c["shape"] and (x >= 0).all()
        keep = x.copy()
        if x.size <= C.STORE_INPUT_MAX:
            out["real/%s/x" % name] = x
        out["real/%s/sha" % name] = np.array(C.sha(x))
        pos = C.kept(x.shape)
        for kernel, power, margin in C.real_runs(name):
            kh, kp = C.pair(kernel)
            assert C.fits(kernel, x.shape), (name, kernel)
            with Recorder(R) as rec:
                mask_h, mask_p = R.hpss(x, kernel_size=kernel, power=power, mask=True, margin=margin)
                (size_h, harm), (size_p, perc) = rec.out
            out_h, out_p = R.hpss(x, kernel_size=kernel, power=power, mask=False, margin=margin)
            assert size_h[-1] == kh and size_p[-2] == kp and set(size_h[:-1]) <= {1} and set(size_p[:-2] + size_p[-1:]) <= {1}
            assert np.array_equal(x, keep)
            for a in (harm, perc, mask_h, mask_p, out_h, out_p):
                assert a.dtype == np.float32 and a.shape == x.shape
            # the window convention, on the reference alone
            assert np.array_equal(harm, C.brute_median(x, kh, -1)) and np.array_equal(perc, C.brute_median(x, kp, -2)), (name, kernel)
            for key, med, k, axis in zip(C.median_keys(name, kernel), (harm, perc), (kh, kp), (-1, -2)):
                off = C.encode(x, med, k, axis)
                assert np.array_equal(C.decode(x, off, k, axis), med)
                assert key not in out or np.array_equal(out[key], off)
                out[key] = off
            assert np.array_equal(out_h, x * mask_h) and np.array_equal(out_p, x * mask_p)
            if c["kind"] == "mix" and x.size >= 1000 and margin == 1.0 and min(kh, kp) >= 17:  # (a 1-tap filter is the identity: masks of 0.5)
                for m in (mask_h, mask_p):
                    assert m.min() < 0.1 and m.max() > 0.9 and ((m > 0.3) & (m < 0.7)).any(), (name, kernel, m.min(), m.max())
            key = C.run_key(name, kernel, power, margin)
            for label, a in (("mask_h", mask_h), ("mask_p", mask_p), ("out_h", out_h), ("out_p", out_p)):
                out["%s/%s" % (key, label)] = a.reshape(-1)[pos]
            print("%-10s k %-6s p %-3g m %-4s  masks in [%.3g, %.3g] [%.3g, %.3g]" % (
                name, C.tag(kernel), power, C.tag(margin), mask_h.min(), mask_h.max(), mask_p.min(), mask_p.max()))
    # the reflections of the short axis really are multiple
    name, kernel = C.MULTI_REFLECTION
    assert kernel in C.REAL_CASES[name]["kernels"] and C.pair(kernel)[1] // 2 > C.REAL_CASES[name]["shape"][-2]

    # ---- soft_mask ----
    for dtype in C.SOFT_DTYPES:
        a, b = C.soft_mask_inputs(dtype)
        tiny = np.finfo(dtype).tiny
        z = np.maximum(a, b)
        assert (z < tiny).sum() >= 8 and ((z >= tiny) & (np.minimum(a, b) < tiny)).sum() >= 16 and (z == tiny).any()
        assert (a == 0).any() and (b == 0).any() and ((a == 0) & (b == 0)).any() and ((a > 0) & (a < tiny)).any()
        assert np.array_equal(a ** 2.0, a * a) and np.array_equal(a ** 1, a) and np.array_equal(a ** 0.5, np.sqrt(a))
        out["soft/%s/a" % dtype], out["soft/%s/b" % dtype] = a, b
        for power in C.POWERS:
            for split_zeros in (False, True):
                keep_a, keep_b = a.copy(), b.copy()
                m = R.soft_mask(a, b, power=power, split_zeros=split_zeros)
                assert np.array_equal(a, keep_a) and np.array_equal(b, keep_b)
                assert m.dtype == (np.bool_ if np.isinf(power) else np.dtype(dtype)) and m.shape == a.shape
                out[C.soft_key(dtype, power, split_zeros)] = m

    # ---- complex spectrograms ----
    for name in C.COMPLEX_SLICES:
        x = C.complex_input(name)
        assert x.dtype == np.complex64 and x.shape == C.COMPLEX_SHAPE
        mag = np.abs(x)
        assert ((mag == 0) | (mag >= C.MAG_FLOOR)).all() and (mag == 0).any()
        out["complex/%s/sha" % name] = np.array(C.sha(x))
        pos = C.kept(x.shape)
        for margin in C.COMPLEX_MARGINS:
            mask_h, mask_p = R.hpss(x, mask=True, margin=margin)
            out_h, out_p = R.hpss(x, mask=False, margin=margin)
            assert mask_h.dtype == np.float32 and out_h.dtype == np.complex64
            key = C.complex_key(name, margin)
            for label, a in (("mask_h", mask_h), ("mask_p", mask_p), ("out_h", out_h), ("out_p", out_p)):
                out["%s/%s" % (key, label)] = a.reshape(-1)[pos]

    # ---- harmonic ----
    had = hasattr(np, "float_")
    if not had:
        np.float_ = np.float64
    try:
        y = C.harmonic_input()
        keep = y.copy()
        ref = R.harmonic(y)
        assert S.stft(y, n_fft=2048, pad_mode="constant").dtype == np.complex64
        S.np = Complex128()
        try:
            assert S.stft(y, n_fft=2048, pad_mode="constant").dtype == np.complex128
            wide = R.harmonic(y)
        finally:
            S.np = np
        assert np.array_equal(y, keep) and ref.shape == wide.shape == y.shape and ref.dtype == np.float64
        frames = S.stft(y, n_fft=2048, pad_mode="constant").shape[-1]
        assert frames >= 8
        e32 = C.errors(ref, wide)
        out["harmonic/x"], out["harmonic/out"], out["harmonic/e32"] = y, ref, np.array(e32)
        print("harmonic: %d samples, %d frames, e32 rms %.3g max %.3g, output rms over input rms %.3g" % (
            len(y), frames, e32[0], e32[1], np.sqrt(np.mean(ref ** 2) / np.mean(y.astype(np.float64) ** 2))))
    finally:
        if not had:
            del np.float_

    np.savez_compressed(C.GOLDENS, **out)
    print(C.GOLDENS, os.path.getsize(C.GOLDENS), "bytes, %d arrays" % len(out))
    assert os.path.getsize(C.GOLDENS) < os.path.getsize(os.path.join(HERE, "processing_goldens.npz"))


if __name__ == "__main__":
    main()
