#!/usr/bin/env python3
"""data.features hpss and harmonic at a training batch's shape: 64 utterances of 10 s at 16 kHz, n_fft = 2048, hop 512 - a
(64, 1025, 313) magnitude batch.

Prints one JSON line with
  hpss / hpss_mask           median_ms of --repeats device-event timings of the whole call on the (64, 1025, 313) float32 device tensor
                             (two median filters, one mask launch per output, the output allocations and the one-flag readback
                             included), min_ms, and must_move_mb / gb_per_s / hbm_frac: the bytes that have to cross HBM whatever the
                             kernels do - the spectrogram read once and the two results written - over median_ms, against the
                             8 TB/s HBM figure of bench.py --full
  hpss_frame_major           the same on the frame-major view that stft returns
  median_time / median_freq  one ma_median_filter launch each (31 taps along time / along frequency, contiguous input), with the
                             bytes of one read and one write, and gcmp_per_s: k^2 compares per output over median_ms
  median_time_fm / median_freq_fm  the same launches on the frame-major view
  soft_mask_out / soft_mask_mask   one ma_soft_mask launch: (harm, perc, spec) -> spec * mask (three reads, one write), and
                             (harm, perc) -> mask (two reads, one write)
  harmonic                   harmonic() on the (64, 160000) float32 waveform batch (stft, magphase, hpss, istft), with the waveform
                             read and written as its must-move bytes
  host_ms                    the reference-style evaluation on this machine's host for ONE utterance, measured: the two
                             scipy.ndimage.median_filter calls and the two soft masks in NumPy on one (1025, 313) slice
  host_batch_ms_extrapolated host_ms times the batch: an extrapolation, labelled as one
Every timing follows warm-up calls; a repeat is one call between two device events after a synchronize.
No threshold: the figures are measurements."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0  # bench.py


def host_reference_style(spec, kernel, power):
    """One utterance the way the reference walks it: two scipy median filters, then the two soft masks in NumPy."""
    from scipy.ndimage import median_filter

    harm = median_filter(spec, size=(1, kernel), mode="reflect")
    perc = median_filter(spec, size=(kernel, 1), mode="reflect")
    outs = []
    for a, b in ((harm, perc), (perc, harm)):
        z = np.maximum(a, b)
        bad = z < np.finfo(np.float32).tiny
        z[bad] = 1
        m, r = (a / z) ** power, (b / z) ** power
        m[~bad] /= m[~bad] + r[~bad]
        m[bad] = 0.5
        outs.append(spec * m)
    return harm, perc, outs


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--kernel", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)

    import torch

    from mindaudio_amd import _host, _lib
    from mindaudio_amd.data import features as F

    n_fft, hop = 2048, 512
    n_freq, frames = n_fft // 2 + 1, a.samples // hop + 1
    rng = np.random.default_rng(0)
    spec_np = (0.2 * rng.random((a.batch, n_freq, frames))).astype(np.float32)
    spec_np[:, rng.choice(n_freq, n_freq // 6, replace=False), :] += 0.7  # steady rows: harmonic
    spec_np[:, :, rng.choice(frames, frames // 6, replace=False)] += 0.7  # loud frames: percussive
    spec = torch.from_numpy(spec_np).cuda()
    spec_fm = spec.transpose(1, 2).contiguous().transpose(1, 2)
    wave = torch.from_numpy((0.1 * rng.standard_normal((a.batch, a.samples))).astype(np.float32)).cuda()
    result = {"batch": a.batch, "n_freq": n_freq, "frames": frames, "samples": a.samples, "kernel": a.kernel, "repeats": a.repeats,
              "device": torch.cuda.get_device_name(0)}

    def timed(fn, nbytes=None, compares=None):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            torch.cuda.synchronize()
            ms.append(start.elapsed_time(end))
        med = statistics.median(ms)
        out = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4)}
        if nbytes:
            out.update(must_move_mb=round(nbytes / 1e6, 2), gb_per_s=round(nbytes / 1e9 / (med * 1e-3), 1),
                       hbm_frac=round(nbytes / 1e9 / (med * 1e-3) / HBM_PEAK_GBS, 4))
        if compares:
            out.update(gcmp_per_s=round(compares / 1e9 / (med * 1e-3), 1))
        return out

    one = spec.numel() * spec.element_size()
    cmp_ = spec.numel() * a.kernel * a.kernel
    result["hpss"] = timed(lambda: F.hpss(spec, kernel_size=a.kernel), 3 * one)
    result["hpss_mask"] = timed(lambda: F.hpss(spec, kernel_size=a.kernel, mask=True), 3 * one)
    result["hpss_frame_major"] = timed(lambda: F.hpss(spec_fm, kernel_size=a.kernel), 3 * one)
    result["median_time"] = timed(lambda: F.median_filter_device(spec, a.kernel, axis=-1), 2 * one, cmp_)
    result["median_freq"] = timed(lambda: F.median_filter_device(spec, a.kernel, axis=-2), 2 * one, cmp_)
    result["median_time_fm"] = timed(lambda: F.median_filter_device(spec_fm, a.kernel, axis=-1), 2 * one, cmp_)
    result["median_freq_fm"] = timed(lambda: F.median_filter_device(spec_fm, a.kernel, axis=-2), 2 * one, cmp_)
    harm = F.median_filter_device(spec, a.kernel, axis=-1)
    perc = F.median_filter_device(spec, a.kernel, axis=-2)
    out = torch.empty_like(spec)
    lib, st = _lib.load(), _host.current_stream_ptr()

    def mask_launch(with_spec):
        _lib.check(lib.ma_soft_mask(_host.ptr(harm), _host.ptr(perc), _lib.DTYPE_F32, spec.numel(), 1.0, 1.0, 2.0, 1,
                                    None if with_spec else _host.ptr(out), _host.ptr(spec) if with_spec else None, None,
                                    _host.ptr(out) if with_spec else None, None, st), "soft_mask")

    result["soft_mask_out"] = timed(lambda: mask_launch(True), 4 * one)
    result["soft_mask_mask"] = timed(lambda: mask_launch(False), 3 * one)
    result["harmonic"] = timed(lambda: F.harmonic(wave, kernel_size=a.kernel), 2 * wave.numel() * wave.element_size())

    got_h, got_p = F.hpss(spec[:1], kernel_size=a.kernel)
    t0 = time.perf_counter()
    h_harm, h_perc, h_outs = host_reference_style(spec_np[0], a.kernel, 2.0)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(h_harm, harm[0].cpu().numpy()) and np.array_equal(h_perc, perc[0].cpu().numpy()), "host and device medians differ"
    assert np.array_equal(h_outs[0], got_h[0].cpu().numpy()) and np.array_equal(h_outs[1], got_p[0].cpu().numpy()), \
        "host and device masked spectrograms differ"
    result["host_ms"] = round(host_ms, 1)
    result["host_batch_ms_extrapolated"] = round(host_ms * a.batch, 1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
