#!/usr/bin/env python3
"""Generate the IIR-filter fixtures by running THE REFERENCE's cal_filter_by_coffs, low_pass_filter, peaking_equalizer and filtfilt
(mindaudio/data/filters.py) in the build container on the cases of tests/iir_cases.py.

Runs only where the reference tree exists; nothing of it travels - its filters module is imported by path behind the `mindspore`
stub of gen_goldens.py, as gen_phase_vocoder_goldens.py does, and only inputs, results and error figures are stored
(tests/golden/iir_goldens.npz; the layout is described in iir_cases.py).

Per case:
  e_in   [relative rms, max-abs over peak] between the reference's float64 result on the float64 input and on that input rounded
         once to float32 (held in a float64 array, so that nothing else is rounded)
  e_re   the largest of the same two figures between the reference's float64 result and other float64 evaluation orders of the
         same recursion: a direct-form-I loop, scipy.signal.lfilter, and iir_cases.chunked (chunk carry in NumPy, P from
         np.linalg.matrix_power) at chunks 64, 256 and 1024 - the candidates that stay finite and on the signal's scale (`spread`).  For filtfilt every candidate runs
         SciPy's own order of operations (odd extension, forward from zi * x_ext[0], backward from zi * y[-1], strip); the
         direct-form-I candidate adds the free response of the initial state, which has no direct-form-I form, from lfilter.
No figure is measured on the code under test.

usage: python tests/golden/gen_iir_goldens.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import iir_cases as C  # noqa: E402


def load_reference():
    spec = importlib.util.spec_from_file_location("gen_goldens", os.path.join(HERE, "gen_goldens.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    gg._install_stubs()
    for name in ("mindaudio", "mindaudio.data"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    return gg._load("mindaudio.data.filters", "mindaudio/data/filters.py")


def spread(ref, candidates):
    """The largest [rms, max] over the candidates that stay finite.  A chunk carry whose matrix power has lost all meaning can stay
    below the overflow threshold and still be 10^100 times the signal: a candidate further from the reference than the reference's
    own peak is no evaluation of the same filter and is dropped with the non-finite ones."""
    e = np.zeros(2)
    for y in candidates:
        if np.all(np.isfinite(y)) and C.errors(y, ref)[1] < 1.0:
            e = np.maximum(e, C.errors(y, ref))
    return e


def chunk_candidates(b, a, run):
    """run(L, P) for the three chunk lengths, P from np.linalg.matrix_power (kept only where it is finite: an overflowing power
    turns the whole evaluation into NaN, which `spread` drops)."""
    A = C.transition(C.padded(b, a)[1])
    for L in (64, 256, 1024):
        with np.errstate(all="ignore"):
            yield run(L, np.linalg.matrix_power(A, L))


def main():
    R = load_reference()
    out = {}
    for case, (fn, args, shape, amp) in C.BIQUAD_CASES.items():
        x64 = C.noise(C.case_seed(case), shape, amp)
        x32 = x64.astype(np.float32)
        ref = getattr(R, fn)(x32.copy(), *args)  # (the reference overwrites its argument)
        ref64 = getattr(R, fn)(x64.copy(), *args)
        ref64r = getattr(R, fn)(x32.astype(np.float64), *args)
        assert ref.dtype == np.float32 and ref64.dtype == ref64r.dtype == np.float64 and ref.shape == x32.shape
        # the coefficients the reference works with: its designers, run on a throw-away sample
        if fn == "cal_filter_by_coffs":
            b, a = args
        else:
            grabbed = {}
            keep = R.cal_filter_by_coffs
            R.cal_filter_by_coffs = lambda w, b_, a_: grabbed.update(b=b_, a=a_) or w
            try:
                getattr(R, fn)(np.zeros(1), *args)
            finally:
                R.cal_filter_by_coffs = keep
            b, a = grabbed["b"], grabbed["a"]
            out[case + "/b"], out[case + "/a"] = b, a
        a1 = np.array([1.0, a[1], a[2]])
        rows = x32.astype(np.float64).reshape(shape[0], -1).T  # (channels, time)
        back = lambda y: np.ascontiguousarray(y.T).reshape(shape)  # noqa: E731
        unclamped = back(scipy.signal.lfilter(b, a1, rows, axis=-1))
        cands = [back(np.minimum(C.direct_form_1(b, a1, rows), 1.0)), np.minimum(unclamped, 1.0)]
        cands += [back(y) for y in chunk_candidates(b, a1, lambda L, P: C.chunked(b, a1, rows, L, P, upper_clamp=True))]
        e_in, e_re = np.array(C.errors(ref64r, ref64)), spread(ref64r, cands)
        if case == C.CLAMP_CASE:
            assert (unclamped > 1.0).any() and (unclamped < -1.0).any(), "the loud case does not cross +1 and -1"
            assert ref.max() == 1.0 and ref.min() < -1.0
            out[case + "/unclamped"] = unclamped
        out[case + "/x"], out[case + "/out"], out[case + "/out64"] = x32, ref, ref64r
        out[case + "/e_in"], out[case + "/e_re"] = e_in, e_re
        print("%-14s %-10s e_in %.2g / %.2g  e_re %.2g / %.2g" % (case, shape, e_in[0], e_in[1], e_re[0], e_re[1]))

    for case, ((N, Wn, btype), shape) in C.FILTFILT_CASES.items():
        x = C.noise(C.case_seed(case), shape, 0.3)
        x32 = x.astype(np.float32).astype(np.float64)
        ref, ref32 = R.filtfilt(x, N, Wn, btype), R.filtfilt(x32, N, Wn, btype)
        assert ref.dtype == ref32.dtype == np.float64 and ref.shape == x.shape
        b, a = scipy.signal.butter(N, Wn, btype)
        zi, padlen = scipy.signal.lfilter_zi(b, a), 3 * max(len(a), len(b))
        rows = x.reshape(-1, shape[-1])
        back = lambda y: y.reshape(shape)  # noqa: E731
        lf = lambda r, z: scipy.signal.lfilter(b, a, r, axis=-1, zi=z)[0]  # noqa: E731
        df1 = lambda r, z: C.direct_form_1(b, a, r) + scipy.signal.lfilter(b, a, np.zeros_like(r), axis=-1, zi=z)[0]  # noqa: E731
        cands = [back(C.filtfilt_with(lf, rows, zi, padlen)), back(C.filtfilt_with(df1, rows, zi, padlen))]
        cands += [back(y) for y in chunk_candidates(b, a, lambda L, P: C.filtfilt_with(
            lambda r, z: C.chunked(b, a, r, L, P, zi=zi, times_x0=True), rows, zi, padlen))]
        assert np.array_equal(cands[0], ref), "filtfilt_with does not reproduce scipy.signal.filtfilt"
        e_in, e_re = np.array(C.errors(ref32, ref)), spread(ref, cands)
        out[case + "/x"], out[case + "/out"], out[case + "/out32"] = x, ref, ref32
        out[case + "/e_in"], out[case + "/e_re"] = e_in, e_re
        print("%-14s %-10s finite candidates %d  e_in %.2g / %.2g  e_re %.2g / %.2g" % (
            case, shape, sum(bool(np.all(np.isfinite(y))) for y in cands), e_in[0], e_in[1], e_re[0], e_re[1]))

    np.savez_compressed(C.GOLDENS, **out)
    print(C.GOLDENS, os.path.getsize(C.GOLDENS), "bytes")
    assert os.path.getsize(C.GOLDENS) < (1 << 20)


if __name__ == "__main__":
    main()
