#!/usr/bin/env python3
"""data.augment.time_stretch at a training batch's shape: 64 waveforms of 10 s (160 000 samples), rates 0.9 and 1.1, n_fft 512, hop 128.

Prints one JSON line with, per rate:
  device_event_ms_stft / _vocoder / _istft   each of the three stages alone (spectrum.stft, augment._phase_vocoder on stft's frame-major
                             memory, spectrum.istft), device events around a window of at least --seconds after warm-up: the stream's
                             wall time per call, host gaps between launches included
  device_event_ms_time_stretch               the whole augment.time_stretch call, same method
  vocoder_must_move_mb / vocoder_gb_per_s    the spectrogram read once and the stretched one written once, from the shapes, over
                             device_event_ms_vocoder
  host_numpy_loop_ms_vocoder                 the reference-style loop over output frames (NumPy, complex64 spectrogram, float32
                             accumulator) on this machine's host for the same batch, one process - to be read against
                             device_event_ms_vocoder
`rocprofv3 --kernel-trace --stats -- python tools/time_stretch_bench.py --once` is the run of its own for the kernel table.
No threshold: the figures are measurements."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_vocoder_loop(spec, rate, hop):
    """The reference's algorithm as it runs it: one pass of whole-array NumPy calls per output frame."""
    steps = np.arange(0, spec.shape[-1], rate, dtype=np.float64)
    out = np.zeros(spec.shape[:-1] + (len(steps),), spec.dtype)
    phi = np.linspace(0, np.pi * hop, spec.shape[-2])
    acc = np.angle(spec[..., 0])
    spec = np.pad(spec, [(0, 0)] * (spec.ndim - 1) + [(0, 2)])
    for t, step in enumerate(steps):
        c0, c1 = spec[..., int(step)], spec[..., int(step) + 1]
        alpha = np.mod(step, 1.0)
        mag = (1.0 - alpha) * np.abs(c0) + alpha * np.abs(c1)
        out[..., t] = mag * (np.cos(acc) + 1j * np.sin(acc))
        d = np.angle(c1) - np.angle(c0) - phi
        d = d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))
        acc += phi + d
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--rates", type=float, nargs="+", default=[0.9, 1.1])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-batch", type=int, default=None, help="rows of the host loop (default: the whole batch)")
    ap.add_argument("--once", action="store_true", help="warm up, run ONE time_stretch per rate and exit (for a kernel trace)")
    a = ap.parse_args(argv)

    import torch

    from mindaudio_amd.data import augment as A
    from mindaudio_amd.data import spectrum as S

    rng = np.random.default_rng(0)
    x = torch.from_numpy((0.1 * rng.standard_normal((a.batch, a.samples))).astype(np.float32)).cuda()
    n_fft, hop = 512, 128
    result = {"batch": a.batch, "samples": a.samples, "n_fft": n_fft, "hop": hop, "device": torch.cuda.get_device_name(0), "rates": {}}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        iters, t0 = 0, time.perf_counter()
        start.record()
        while True:
            fn()
            iters += 1
            if iters % 8 == 0:
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= a.seconds:
                    break
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters, iters

    for rate in a.rates:
        length = int(round(a.samples / rate))
        if a.once:
            for _ in range(a.warmup + 1):
                A.time_stretch(x, rate)
            torch.cuda.synchronize()
            continue
        spec = S.stft(x)
        stretched = A._phase_vocoder(spec, rate)
        ms_stft, _ = timed(lambda: S.stft(x))
        ms_voc, it_voc = timed(lambda: A._phase_vocoder(spec, rate))
        ms_istft, _ = timed(lambda: S.istft(stretched, length=length))
        ms_all, it_all = timed(lambda: A.time_stretch(x, rate))
        nbytes = 8 * spec.shape[0] * spec.shape[1] * (spec.shape[2] + stretched.shape[2])
        hb = a.host_batch or a.batch
        spec_host = spec[:hb].cpu().numpy()
        t0 = time.perf_counter()
        host_vocoder_loop(spec_host, rate, hop)
        host_ms = (time.perf_counter() - t0) * 1e3
        result["rates"]["%g" % rate] = {
            "frames": spec.shape[2], "steps": stretched.shape[2], "out_samples": length,
            "device_event_ms_stft": round(ms_stft, 4), "device_event_ms_vocoder": round(ms_voc, 4),
            "device_event_ms_istft": round(ms_istft, 4), "device_event_ms_time_stretch": round(ms_all, 4),
            "iters_vocoder": it_voc, "iters_time_stretch": it_all,
            "vocoder_must_move_mb": round(nbytes / 1e6, 2), "vocoder_gb_per_s": round(nbytes / 1e9 / (ms_voc * 1e-3), 1),
            "host_numpy_loop_ms_vocoder": round(host_ms, 1), "host_rows": hb,
        }
    if not a.once:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
