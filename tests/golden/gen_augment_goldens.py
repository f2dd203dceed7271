#!/usr/bin/env python3
"""Generate tests/golden/augment_goldens.npz by running THE REFERENCE's augmenters (mindaudio/data/augment.py and the helpers it
imports: io, spectrum, filters, processing) in the build container, on the cases of tests/augment_cases.py.

Runs only where the reference tree exists; nothing of it travels - the reference modules are imported by path as a fake
`mindaudio.data` package behind the `mindspore` stub of gen_goldens.py, and only inputs' recipes, decisions and outputs are stored.

Per case the fixture holds
  <case>/out    the reference's float64 output (float32 where the result is derivable bit for bit; sampled columns for the one
                full-size case), flattened to (rows, time)
  <case>/draws  JSON: every np.random.rand / randint / uniform and random.choice call the reference made after
                np.random.seed(s); random.seed(s) - name, arguments, result - and the next draw of both generators
  <case>/e32    [relative rms, max-abs over peak] of a SINGLE-PRECISION CPU evaluation of the same formula (float32 arrays, scipy.fft,
                which stays in single precision) against <case>/out: what float32 costs on the reference's formula, the yardstick of
                test_augment_gpu.py.  Never measured on the code under test.
plus notch/<f> (filters.notch_filter) and drop_filter/<case> (the composed filter of the drop_freq cases) in float64.

usage: python tests/golden/gen_augment_goldens.py
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import scipy.fft as sfft
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import augment_cases as C  # noqa: E402


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    gg = _by_path("gen_goldens", os.path.join(HERE, "gen_goldens.py"))
    gg._install_stubs()
    for name in ("mindaudio", "mindaudio.data"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    mods = {}
    for m in ("io", "spectrum", "filters", "processing", "augment"):
        mods[m] = gg._load("mindaudio.data." + m, "mindaudio/data/%s.py" % m)
    return mods


flat, TIME_AXIS = C.flat, C.TIME_AXIS


# ---- single-precision evaluations of the reference's formulas -------------------------------------------------------------------------
F = np.float32


def conv32(x, h, rot=0):
    """x (rows, T) float32, h float32 taps: convolve1d(use_fft=True) in single precision."""
    t = x.shape[-1]
    h = h[:t]
    k = np.zeros(t, F)
    after = h[rot:]
    k[:after.shape[0]] = after
    if rot:
        k[t - min(rot, h.shape[0]):] = h[:rot]
    return sfft.irfft(sfft.rfft(x) * sfft.rfft(k), n=t)


def reverb32(x, h):
    rot = int(np.argmax(np.abs(h)))
    n = F(x.shape[-1])
    amp = np.abs(x).sum(axis=-1, keepdims=True, dtype=F) / n
    y = conv32(x, h, rot)
    return y / (np.abs(y).sum(axis=-1, keepdims=True, dtype=F) / n + F(1e-14)) * amp


def noise32(x, background, snr):
    rms = np.sqrt(np.square(x).mean(axis=-1, keepdims=True, dtype=F))
    return x + background.astype(F)[None, :] * (rms / F(10 ** (snr / 20)))


def background64(io, paths, n):
    pieces, missing = None, n
    norm = lambda s: s / (np.sqrt(np.square(s).mean(keepdims=True)) + 1e-8)  # noqa: E731
    for p in paths:
        a, _ = io.read(p)
        piece = norm(a[:missing]) if len(a) > missing else norm(a)
        missing -= min(len(a), missing)
        pieces = piece if pieces is None else np.append(pieces, piece)
    return norm(pieces.reshape(1, n))[0]


def babble32(x, lengths, speakers, snr):
    lens = (lengths * x.shape[1])[:, None].astype(F)
    amp = np.abs(x).sum(axis=1, keepdims=True, dtype=F) / lens
    f = (1 / (10.0 ** (0.1 * snr) + 1)).astype(F)
    new_amp = f * amp
    out = x * (F(1) - f)
    bab = np.roll(x, 1, axis=0)
    blen = np.roll(lens, 1, axis=0)
    for i in range(1, speakers):
        bab = bab + np.roll(x, 1 + i, axis=0)
        blen = np.maximum(blen, np.roll(blen, 1, axis=0))
    bamp = np.abs(bab).sum(axis=1, keepdims=True, dtype=F) / blen
    return out + bab * (new_amp / (bamp + F(1e-14)))


def draws_of(log, name):
    return [e for e in log if e[0] == name]


def drop_chunk32(x, lens, dec, noise_factor):
    """dec: the host decisions (our drop_chunk_host replayed on the recorded seed and checked against the reference's log)."""
    y = x.copy()
    amp = np.abs(x).sum(axis=1, dtype=F) / (lens * x.shape[1]).astype(F)
    for i in range(x.shape[0]):
        for j in range(len(dec["length"][i])):
            lo, hi = dec["intervals"][i, j]
            if noise_factor:
                m = F(2) * amp[i] * F(noise_factor)
                u = dec["fill"][dec["fill_off"][i, j]:dec["fill_off"][i, j] + hi - lo]
                y[i, lo:hi] = F(2) * m * u - m
            else:
                y[i, lo:hi] = 0
    return y


def main():
    ref = load_reference()
    R, io = ref["augment"], ref["io"]
    from mindaudio_amd.data import augment as A  # host halves only (no device): decisions for the float32 evaluations

    w, sr = io.read(C.WAV)
    assert sr == 16000 and np.array_equal(w, C.wav())  # the two readers agree on the fixture's source
    out = {}
    for fq in (0.1, 0.25, 0.73):
        out["notch/%g" % fq] = ref["filters"].notch_filter(fq)
    with tempfile.TemporaryDirectory() as tmp:
        files = C.make_files(tmp)

        def host(name):
            with C.record_draws(C.CASES[name]["seed"]) as rec:
                dec = C.CASES[name]["host"](A, files)
            return dec, rec.log

        def e32_of(name):
            x = {k: getattr(C, k)() for k in dir(C) if k.startswith(("X_", "K_", "L_"))}
            if name.startswith("drop_freq"):
                dec, _ = host(name)
                xin = x["X_DF1"] if name.endswith("1") else x["X_DF2"]
                out["drop_filter/" + name] = dec["filter"]
                return conv32(flat(xin, 1 if xin.ndim == 3 else -1), dec["filter"].astype(F))
            if name == "conv_rot":
                return conv32(x["X_CV1"], x["K_CV1"], 37)
            if name == "conv_long_kernel":
                return conv32(x["X_CV2"][None], x["K_CV2"], 5)
            if name == "conv_odd":
                return conv32(flat(x["X_CV3"], 1), x["K_CV3"])
            if name == "reverb_1d":
                return reverb32(x["X_RV1"][None], x["K_RV"])
            if name == "reverb_bt1":
                return reverb32(flat(x["X_RV2"], 1), x["K_RV"])
            if name == "reverb_big":
                return reverb32(flat(x["X_BIG"], 1), x["K_BIG"])
            if name.startswith("add_reverb"):
                dec, _ = host(name)
                xin = x["X_AR1"] if name.endswith("bt") else x["X_AR2"]
                return reverb32(flat(xin, -1), dec["rir"].astype(F))
            if name.startswith("add_noise"):
                dec, _ = host(name)
                xin = x["X_AN1"] if name.endswith("cut") else x["X_AN2"]
                return noise32(xin, dec["background"], dec["snr"])
            if name == "add_babble":
                dec, _ = host(name)
                return babble32(x["X_BB"], x["L_BB"], 3, dec["snr"])
            if name.startswith("drop_chunk"):
                dec, _ = host(name)
                xin, lens = (x["X_DC0"], np.ones(4)) if name.endswith("count0") else (x["X_DC"], x["L_DC"])
                return drop_chunk32(xin, lens, dec, 0.5 if name.endswith("noise") else 0.0)
            if name.startswith("speed_"):
                sp = int(name.split("_")[1])
                if sp == 100:
                    return x["X_SP"]
                return scipy.signal.resample(x["X_SP"], int(np.ceil(1600 * (float(16000 * sp // 100) / 16000))), axis=-1).astype(F)
            if name == "chain_time_domain":
                (idx, df, dc), _ = host(name)
                sp = [95, 100, 105][idx]
                y = x["X_T"]
                if sp != 100:
                    y = scipy.signal.resample(y, int(np.ceil(3200 * (float(16000 * sp // 100) / 16000))), axis=-1).astype(F)
                y = conv32(y, df["filter"].astype(F))
                return drop_chunk32(y, np.ones(2), dc, 0.0)
            if name == "chain_env_corrupt":
                (rv, nz), _ = host(name)
                return noise32(reverb32(x["X_E"], rv["rir"].astype(F)), nz["background"], nz["snr"])
            raise KeyError(name)

        for name, case in C.CASES.items():
            with C.record_draws(case["seed"]) as rec:
                y = case["ref"](R, files)
            y = flat(y, TIME_AXIS.get(name, -1))
            assert y.dtype == np.float64, (name, y.dtype)
            if case.get("host"):  # our host halves take the reference's decisions: the float32 evaluation below relies on it
                _, log = host(name)
                assert log == rec.log, (name, log[:6], rec.log[:6])
            y32 = np.asarray(e32_of(name))
            assert y32.dtype == np.float32 and y32.shape == y.shape, (name, y32.dtype, y32.shape, y.shape)
            if name == "drop_chunk_count0":
                assert 0 in [int(v) for v in rec.log[1][2]], "pick a seed for which some row draws no chunk"
            if case.get("cols") is not None:
                cols = case["cols"]()
                y, y32 = y[:, cols], y32[:, cols]
            err = y32.astype(np.float64) - y
            e32 = [float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(y ** 2))), float(np.abs(err).max() / np.abs(y).max())]
            if case.get("exact"):
                assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and e32 == [0.0, 0.0], name
                y = y.astype(np.float32)
            out[name + "/out"] = y
            out[name + "/e32"] = np.array(e32)
            out[name + "/draws"] = np.array(json.dumps(rec.log))
            print("%-22s out %-12s e32 rms %.3g max %.3g  draws %d" % (name, y.shape, e32[0], e32[1], len(rec.log) - 1))
    path = os.path.join(HERE, "augment_goldens.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
