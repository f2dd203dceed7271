#!/usr/bin/env python3
"""Generate tests/golden/separation_sisnr.npz by running THE REFERENCE's cal_SISNR and cal_SISNRi (mindaudio/metric/snr.py) on a
handful of seeded float32 signal pairs of at most 1000 samples.

Runs only where the reference tree exists; nothing of it travels - the module is imported by path with a stub
`mir_eval.separation` in sys.modules (snr.py imports bss_eval_sources at the top; cal_SDRi, which needs it, is not called), and only
inputs and results are stored.  The signals are handed to the reference as float64 copies of the stored float32 arrays, so that its
arithmetic runs in float64 whatever NumPy's scalar promotion rules are.

  ref<i>, est<i>   float32 (T,) - the pairs of cal_SISNR; sisnr (n,) float64 - the reference's results, in order
                   (a generic pair, a short one, a scaled estimate, a silent reference, an estimate equal to the reference,
                   the reference plus -60 dB noise)
  src_ref, src_est (2, T) float32, mix (T,) float32, sisnri () float64 - one cal_SISNRi case
No figure is measured on the code under test.

usage: python tests/golden/gen_separation_goldens.py [reference root]
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(root):
    stub = types.ModuleType("mir_eval.separation")
    stub.bss_eval_sources = None
    pkg = types.ModuleType("mir_eval")
    pkg.separation = stub
    sys.modules["mir_eval"], sys.modules["mir_eval.separation"] = pkg, stub
    spec = importlib.util.spec_from_file_location("reference_snr", os.path.join(root, "mindaudio", "metric", "snr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MINDAUDIO_REFERENCE", "/root/reference")
    R = load_reference(root)
    rng = np.random.RandomState(20240)
    f32 = np.float32
    pairs = []
    a = rng.randn(1000).astype(f32)
    pairs.append((a, (0.7 * a + 0.3 * rng.randn(1000)).astype(f32)))                 # generic
    b = rng.randn(37).astype(f32)
    pairs.append((b, rng.randn(37).astype(f32)))                                      # short, unrelated
    c = (rng.randn(1000) + 0.5).astype(f32)
    pairs.append((c, (-3.0 * c + 0.05 * rng.randn(1000)).astype(f32)))               # scaled, sign flipped, with an offset
    pairs.append((np.zeros(500, f32), rng.randn(500).astype(f32)))                    # silent reference
    d = rng.randn(1000).astype(f32)
    pairs.append((d, d.copy()))                                                       # estimate equal to the reference
    e = rng.randn(1000).astype(f32)
    pairs.append((e, (e + 1e-3 * rng.randn(1000)).astype(f32)))                       # the reference plus -60 dB noise
    out = {}
    vals = []
    for i, (ref, est) in enumerate(pairs):
        out["ref%d" % i], out["est%d" % i] = ref, est
        vals.append(float(R.cal_SISNR(ref.astype(np.float64), est.astype(np.float64))))
    out["sisnr"] = np.asarray(vals, np.float64)
    s = rng.randn(2, 800).astype(f32)
    mix = (s[0] + s[1]).astype(f32)
    est = (s + 0.2 * rng.randn(2, 800)).astype(f32)
    out["src_ref"], out["src_est"], out["mix"] = s, est, mix
    out["sisnri"] = np.float64(R.cal_SISNRi(s.astype(np.float64), est.astype(np.float64), mix.astype(np.float64)))
    path = os.path.join(HERE, "separation_sisnr.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes;", "sisnr", np.round(out["sisnr"], 3), "sisnri", round(float(out["sisnri"]), 3))


if __name__ == "__main__":
    main()
