#!/usr/bin/env python3
"""data.processing trim_batch, split_batch and normalize at a training batch's shape: 64 waveforms of 10 s at 16 kHz, frames of
2048 samples every 512.

Prints one JSON line with
  trim_batch / split_batch   median_ms of --repeats device-event timings of the whole call on a (64, 160000) float32 device tensor
                             (frame power, row maximum, edges: three launches, the output allocations included), min_ms, and
                             must_move_mb / gb_per_s / hbm_frac: the batch read once, from the shapes, over median_ms, against the
                             8 TB/s HBM figure of bench.py --full
  frame_power / silence_edges  the same for the two C entries alone on preallocated outputs
  normalize                  normalize(x, "max", axis=1) and axis=0 on the same array (one statistics launch and the division)
  host_frame_ms              the reference-style evaluation on this machine's host for ONE row of the batch, measured: the padded
                             row framed into a (frame_length, frames) float64 array by a Python loop of frame_length slices, then
                             mean(|x|^2), the decibels and the edges in NumPy
  host_batch_ms_extrapolated  host_frame_ms times the batch: an extrapolation, labelled as one
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


def host_frame_style(row, top_db, frame_length, hop_length):
    """One row the way the reference walks it: pad, frame by a loop over the frame's samples, power, decibels, edges."""
    x = np.pad(row, frame_length // 2)
    frames = (x.shape[-1] - frame_length) // hop_length + 1
    framed = np.zeros((frame_length, frames))
    for i in range(frame_length):
        framed[i, :] = x[i:i + frames * hop_length][::hop_length]
    power = np.sqrt(np.mean(np.abs(framed) ** 2, axis=0)) ** 2
    db = 10.0 * np.log10(np.maximum(power, 1e-10)) - 10.0 * np.log10(max(1e-10, power.max()))
    flags = np.concatenate([[False], db > -top_db, [False]])
    return np.flatnonzero(flags[1:] != flags[:-1]) * hop_length


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--frame-length", type=int, default=2048)
    ap.add_argument("--hop-length", type=int, default=512)
    ap.add_argument("--top-db", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args(argv)

    import torch

    from mindaudio_amd.data import processing as P

    rng = np.random.default_rng(0)
    level = np.where((np.arange(a.samples) // 16000) % 2 == 0, 0.3, 1e-4)  # a second of signal, a second of near silence
    x_np = ((2.0 * rng.random((a.batch, a.samples)) - 1.0) * level).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    fl, hop = a.frame_length, a.hop_length
    result = {"batch": a.batch, "samples": a.samples, "frame_length": fl, "hop_length": hop, "repeats": a.repeats,
              "device": torch.cuda.get_device_name(0)}

    def timed(fn, nbytes=None):
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
        return out

    nbytes = x.numel() * x.element_size()
    kw = dict(top_db=a.top_db, frame_length=fl, hop_length=hop)
    result["trim_batch"] = timed(lambda: P.trim_batch(x, None, **kw), nbytes)
    result["split_batch"] = timed(lambda: P.split_batch(x, None, **kw), nbytes)
    result["frame_power"] = timed(lambda: P.frame_power_device(x, None, fl, hop), nbytes)
    power, row_max = P.frame_power_device(x, None, fl, hop)
    result["silence_edges"] = timed(lambda: P.silence_edges_device(power, row_max, a.samples, None, fl, hop, a.top_db, None))
    result["normalize_max_axis1"] = timed(lambda: P.normalize(x, "max", axis=1), 2 * nbytes)
    result["normalize_max_axis0"] = timed(lambda: P.normalize(x, "max", axis=0), 2 * nbytes)
    result["normalize_mean_std_axis1"] = timed(lambda: P.normalize(x, "mean_std", axis=1))
    counts, edges = P.split_batch(x, None, **kw)
    m = int(counts[0])
    t0 = time.perf_counter()
    host = host_frame_style(x_np[0], a.top_db, fl, hop)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(np.minimum(host, a.samples), edges[0, :2 * m].cpu().numpy()), "host and device disagree on row 0"
    result["intervals_row0"] = m
    result["host_frame_ms"] = round(host_ms, 2)
    result["host_batch_ms_extrapolated"] = round(host_ms * a.batch, 1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
