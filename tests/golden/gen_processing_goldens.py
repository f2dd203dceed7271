#!/usr/bin/env python3
"""Generate the data.processing fixtures by running THE REFERENCE's trim, split, normalize, stereo_to_mono, invert_channels, loop,
clip and insert_in_background (mindaudio/data/processing.py, with frame and amplitude_to_dB of mindaudio/data/spectrum.py) in the
build container on the cases of tests/processing_cases.py.

Runs only where the reference tree exists; nothing of it travels - its modules are imported by path behind the `mindspore` stub of
gen_goldens.py, as gen_iir_goldens.py does, and only inputs, results and error figures are stored
(tests/golden/processing_goldens.npz; the layout is described in processing_cases.py).

trim / split: the reference's own intermediate rows are taken by wrapping the amplitude_to_dB its processing module calls - what
goes in is np.sqrt(power) ** 2, what comes out is the decibel row - and the generator asserts that every frame of every case lies at
least MARGIN_DB from the threshold -top_db, so that the on/off decision cannot hinge on a rounding.
normalize: `spread` is the largest difference over the peak between the reference's result and the reference run again with its
NumPy handle replaced by one whose sum / mean / std add in reversed order, and by one that adds with math.fsum.
No figure is measured on the code under test.

usage: python tests/golden/gen_processing_goldens.py
"""
import contextlib
import importlib.util
import io
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import processing_cases as C  # noqa: E402


def load_reference():
    spec = importlib.util.spec_from_file_location("gen_goldens", os.path.join(HERE, "gen_goldens.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    gg._install_stubs()
    for name in ("mindaudio", "mindaudio.data"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    gg._load("mindaudio.data.spectrum", "mindaudio/data/spectrum.py")
    return gg._load("mindaudio.data.processing", "mindaudio/data/processing.py")


class Recorder:
    """Wraps the amplitude_to_dB the reference's processing module calls and keeps what went in and what came out."""

    def __init__(self, module):
        self.module, self.inner = module, module.amplitude_to_dB

    def __enter__(self):
        self.module.amplitude_to_dB = self
        return self

    def __exit__(self, *exc):
        self.module.amplitude_to_dB = self.inner
        return False

    def __call__(self, rms, **kw):
        self.rms = np.array(rms, np.float64)
        self.db = self.inner(rms, **kw)
        return self.db


class SumOrder:
    """A stand-in for the reference module's `np`: everything is NumPy's, except that sum, mean and std of a float array add along
    the axis in the order `line_sum` gives."""

    def __init__(self, line_sum):
        self._line_sum = line_sum

    def __getattr__(self, name):
        return getattr(np, name)

    def sum(self, a, axis=None, keepdims=False, dtype=None):
        a = np.asarray(a, dtype if dtype is not None else None)
        if a.dtype != np.float64:
            a = a.astype(np.float64)
        out = np.apply_along_axis(self._line_sum, axis, a)
        return np.expand_dims(out, axis) if keepdims else out

    def mean(self, a, axis=None, keepdims=False):
        return self.sum(a, axis=axis, keepdims=keepdims) / np.shape(a)[axis]

    def std(self, a, axis=None, keepdims=False):
        dev = np.abs(a - self.mean(a, axis=axis, keepdims=True)) ** 2
        return np.sqrt(self.mean(dev, axis=axis, keepdims=keepdims))


def reversed_sum(line):
    acc = 0.0
    for v in line[::-1]:
        acc += v
    return acc


def main():
    R = load_reference()
    out = {}
    smallest = np.inf
    # ---- trim / split ----
    for name, c in C.SILENCE_CASES.items():
        x = C.silence_signal(name)
        kw = dict(top_db=c["top_db"], reference=C.reference_arg(c), frame_length=c["frame_length"], hop_length=c["hop_length"])
        keep = x.copy()
        with Recorder(R) as rec:
            try:
                trimmed, index = R.trim(x, **kw)
                assert np.array_equal(trimmed, x[index[0]:index[1]])
                out[name + "/trim_index"] = np.asarray(index, np.int64)
            except Exception as exc:  # the reference's own failure: its type is what the mirror must raise
                out[name + "/trim_error"] = np.array(type(exc).__name__)
            rms, db = rec.rms, np.array(rec.db, np.float64)
            intervals = R.split(x, **kw)
            assert np.array_equal(rec.rms, rms)
        assert np.array_equal(x, keep)
        n = x.shape[0]
        assert rms.shape == (C.num_frames(n, c["frame_length"], c["hop_length"]),)
        margin = float(np.abs(db + c["top_db"]).min())
        assert margin >= C.MARGIN_DB, (name, margin)
        smallest = min(smallest, margin)
        out[name + "/x"], out[name + "/power"], out[name + "/db"] = x, rms, db
        out[name + "/flags"], out[name + "/margin"] = db > -c["top_db"], np.array(margin)
        out[name + "/split"] = np.asarray(intervals, np.int64).reshape(-1, 2)
        print("%-22s n %-6d frames %-4d margin %.3g dB  trim %s  split %d" % (
            name, n, len(rms), margin, out.get(name + "/trim_index", out.get(name + "/trim_error")), len(intervals)))
    assert str(out[C.NONE_PASS_CASE + "/trim_error"]) == "IndexError" and not out[C.NONE_PASS_CASE + "/flags"].any()
    out["smallest_margin"] = np.array(smallest)
    print("smallest margin over the silence cases: %.3g dB" % smallest)

    # ---- normalize ----
    orders = (SumOrder(reversed_sum), SumOrder(lambda line: math.fsum(line)))
    for name in C.NORM_SHAPES:
        out["norm/%s/x" % name] = C.normalize_input(name)
    worst = 0.0
    for name, axis, norm, dtype in C.normalize_cases():
        x = C.cast(out["norm/%s/x" % name], dtype)
        keep = x.copy()
        ref = R.normalize(x, norm=norm, axis=axis)
        assert np.array_equal(x, keep) and ref.shape == x.shape
        key = C.norm_key(name, axis, norm, dtype)
        pos = C.kept(x.shape)
        out[key] = ref.reshape(-1)[pos]
        if norm not in C.EXACT_NORMS:
            spread = 0.0
            for order in orders:
                R.np = order
                try:
                    alt = R.normalize(x, norm=norm, axis=axis)
                finally:
                    R.np = np
                assert alt.dtype == ref.dtype
                spread = max(spread, C.peak_error(alt, ref))
            out[key + "/spread"] = np.array(spread)
            worst = max(worst, spread)
    print("normalize: %d cases, largest spread between summation orders %.3g" % (len(list(C.normalize_cases())), worst))

    # ---- stereo_to_mono ----
    for name in C.MONO_CASES:
        x = C.mono_input(name)
        y = R.stereo_to_mono(x)
        out[name + "/x"], out[name + "/out"] = x, y
    # ---- indexing ----
    for name, (fn, args) in C.INDEX_CASES.items():
        call = [a.copy() if isinstance(a, np.ndarray) else a for a in args]  # (invert_channels works in place)
        with contextlib.redirect_stdout(io.StringIO()) as said:
            y = getattr(R, fn)(*call)
        for k, a in enumerate(args):
            if isinstance(a, np.ndarray):
                out["%s/arg%d" % (name, k)] = a
        out[name + "/out"], out[name + "/printed"] = np.asarray(y), np.array(said.getvalue())

    np.savez_compressed(C.GOLDENS, **out)
    print(C.GOLDENS, os.path.getsize(C.GOLDENS), "bytes")
    assert os.path.getsize(C.GOLDENS) < (1 << 20)


if __name__ == "__main__":
    main()
