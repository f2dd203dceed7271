#!/usr/bin/env python3
"""ECAPA training-data generation at the example's shape: B = 32 chunks of 48 000 samples, five augmenters (two
TimeDomainSpecAugment, three EnvCorrupt), fbank(80 mels, n_fft 400, hop 160) and sentence mean normalisation.

Prints one JSON line with, per batch:
  device_event_ms_batch      ecapa.generate_train_data.augment_batch (augmenters + fbank + normalisation), device events around a
                             window of at least --seconds after warm-up: the stream's wall time, host gaps between launches included
  device_event_ms_augment    the five augmenters alone (every construct(...) writing its slice of the (6B, N) matrix), same method
  kernel_launches_batch      device kernels of one augment_batch call, counted by torch.profiler (null when the profiler gives none;
                             `rocprofv3 --kernel-trace --stats -- python tools/augment_bench.py --once` is the run of its own for
                             the kernel table)
  must_move_mb / gb_per_s    the bytes the chain has to move, from the shapes (see must_move_bytes), over device_event_ms_batch
  host_numpy_f64_ms_augment  the same five augmenters restated in NumPy / SciPy float64 on this machine's host, one process, with the
                             same decisions - to be read against device_event_ms_augment
The impulse responses and noises are seeded synthetic arrays written as 16-bit WAVs into a temporary folder; the speech is seeded
noise.  No threshold: the figures are measurements."""
import argparse
import json
import os
import random
import sys
import tempfile
import time
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _write_wav(path, samples):
    pcm = np.clip(np.round(samples * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as fh:
        fh.setnchannels(1)
        fh.setsampwidth(2)
        fh.setframerate(16000)
        fh.writeframes(pcm.tobytes())


def make_folder(folder, rng, rir_taps):
    noise, rirs = [], []
    for k in range(4):
        path = os.path.join(folder, "noise_%d.wav" % k)
        _write_wav(path, 0.1 * rng.standard_normal(48000))  # openrir_max_noise_len: 3 s
        noise.append(path)
    for k in range(4):
        r = rng.standard_normal(rir_taps) * np.exp(-np.abs(np.arange(rir_taps) - 120.0) / (rir_taps / 8.0)) * 0.05
        r[120] = 0.9
        path = os.path.join(folder, "rir_%d.wav" % k)
        _write_wav(path, r)
        rirs.append(path)
    for name, paths in (("noise.csv", noise), ("reverb.csv", rirs)):
        with open(os.path.join(folder, name), "w") as fh:
            fh.write("ID,duration,wav,wav_format,wav_opts\n\n")
            for p in paths:
                fh.write(",".join((os.path.basename(p)[:-4], "3.0", p, "wav", "\n")))


def must_move_bytes(b, n, n_aug=5, frames=301, mels=80):
    """Every augmenter reads the clean batch and writes its slice; the clean batch is copied; the fbank reads the matrix and writes the
    features; the normalisation reads and writes them."""
    wave_bytes = b * n * 4
    feat_bytes = (1 + n_aug) * b * frames * mels * 4
    return 2 * n_aug * wave_bytes + 2 * wave_bytes + (1 + n_aug) * wave_bytes + 3 * feat_bytes


def host_chain_f64(x, augs):
    """The five augmenters in NumPy / SciPy float64, decisions from the host halves of data.augment (same generators, same order)."""
    import scipy.signal

    from mindaudio_amd.data import augment as A

    b, n = x.shape
    out = [x]

    def fit(w):
        y = np.zeros((b, n))
        m = min(n, w.shape[1])
        y[:, :m] = w[:, :m]
        return y

    def circ(w, taps, rot=0):
        t = w.shape[1]
        k = np.zeros(t)
        k[:taps.shape[0]] = taps
        return np.fft.irfft(np.fft.rfft(w) * np.fft.rfft(np.roll(k, -rot)), n=t)

    def reverb(w, dec):
        taps, rot = A.reverberate_host(dec["rir"], w.shape[1])
        y = circ(w, taps, rot)
        return y / (np.abs(y).mean(axis=1, keepdims=True) + 1e-14) * np.abs(w).mean(axis=1, keepdims=True)

    def noise(w, dec):
        return w + dec["background"][None, :] * (np.sqrt(np.square(w).mean(axis=1, keepdims=True)) / 10 ** (dec["snr"] / 20))

    for aug in augs[:2]:
        w = x
        idx = A.speed_perturb_host(len(aug.speeds))
        if idx is not None and aug.speeds[idx] != 100:
            w = scipy.signal.resample(w, int(np.ceil(n * (16000 * aug.speeds[idx] // 100) / 16000)), axis=-1)
        w = circ(w, A.drop_freq_host()["filter"])
        dec = A.drop_chunk_host(np.ones(b), w.shape[1], b)
        w = w.copy()
        for i in range(b):
            for lo, hi in dec["intervals"][i]:
                w[i, lo:hi] = 0.0
        out.append(fit(w))
    for aug in augs[2:]:
        w = x
        if hasattr(aug, "add_reverb"):
            w = reverb(w, A.add_reverb_host(aug.add_reverb.rir_data, 1.0))
        if hasattr(aug, "add_noise"):
            w = noise(w, A.add_noise_host(n, aug.add_noise.noise_data, aug.add_noise.snr_low, aug.add_noise.snr_high, 1.0))
        out.append(w)
    return np.concatenate(out, axis=0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--rir-taps", type=int, default=16000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="warm up, run ONE augment_batch and exit (for a kernel trace)")
    a = ap.parse_args(argv)

    import torch

    from mindaudio_amd.ecapa.generate_train_data import augment_batch, default_augmenters

    rng = np.random.default_rng(0)
    b, n = a.batch, a.samples
    x_host = (0.1 * rng.standard_normal((b, n))).astype(np.float32)
    with tempfile.TemporaryDirectory() as folder:
        make_folder(folder, rng, a.rir_taps)
        augs = default_augmenters(folder)
        x = torch.from_numpy(x_host).cuda()
        lens = np.ones(b)
        mat = torch.empty((6 * b, n), dtype=torch.float32, device="cuda")

        def seed(s):
            np.random.seed(s)
            random.seed(s)

        def augment_only():
            mat[:b].copy_(x)
            for k, aug in enumerate(augs):
                aug.construct(x, lens, out=mat[(k + 1) * b:(k + 2) * b])

        for i in range(a.warmup):
            seed(i)
            augment_batch(x, augs)
            augment_only()
        torch.cuda.synchronize()
        if a.once:
            seed(100)
            augment_batch(x, augs)
            torch.cuda.synchronize()
            return

        def timed(fn):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            iters, t0 = 0, time.perf_counter()
            start.record()
            while True:
                seed(1000 + iters)
                fn()
                iters += 1
                if iters % 8 == 0:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= a.seconds:
                        break
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end) / iters, iters

        ms_batch, it_batch = timed(lambda: augment_batch(x, augs))
        ms_aug, it_aug = timed(augment_only)

        launches = None
        try:
            from torch.profiler import ProfilerActivity, profile

            seed(100)
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                augment_batch(x, augs)
                torch.cuda.synchronize()
            n_k = sum(1 for e in prof.events() if "kernel" in str(getattr(e, "device_type", "")).lower() or
                      str(getattr(e, "device_type", "")).endswith("CUDA"))
            launches = n_k or None
        except Exception:
            launches = None

        x64 = x_host.astype(np.float64)
        host_ms = []
        for i in range(3):
            seed(2000 + i)
            t0 = time.perf_counter()
            host_chain_f64(x64, augs)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        nbytes = must_move_bytes(b, n)
        print(json.dumps({
            "batch": b, "samples": n, "rir_taps": a.rir_taps, "device": torch.cuda.get_device_name(0),
            "device_event_ms_batch": round(ms_batch, 4), "iters_batch": it_batch,
            "device_event_ms_augment": round(ms_aug, 4), "iters_augment": it_aug,
            "kernel_launches_batch": launches,
            "must_move_mb": round(nbytes / 1e6, 2), "gb_per_s": round(nbytes / 1e9 / (ms_batch * 1e-3), 1),
            "host_numpy_f64_ms_augment": round(min(host_ms), 2),
        }))


if __name__ == "__main__":
    main()
