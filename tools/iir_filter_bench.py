#!/usr/bin/env python3
"""data.filters.low_pass_filter and filtfilt(4, 0.1, 'lowpass') at a training batch's shape: 64 waveforms of 10 s at 16 kHz.

Prints one JSON line with, per function:
  device_event_ms            the whole call on device tensors (low_pass_filter: a (160000, 64) float32 time-first batch, its two
                             transposes included; filtfilt: (64, 160000) float32, both passes in float64), device events around a
                             window of at least --seconds after warm-up: the stream's wall time per call, host gaps included
  kernel                     ma_iir_filter alone on rows already laid out (float32 for the biquad, float64 for a filtfilt pass), per
                             chunk length of --chunks: device_event_ms, and the same call restricted to each of its three launches
                             (chunk states, carry, emit - the workspace holds the states of a whole call) with each one's share of
                             their sum; must_move_mb / gb_per_s / hbm_frac: the samples read twice and written once, from the
                             shapes, over device_event_ms, against the 8 TB/s HBM figure of bench.py --full
  host_scipy_ms              scipy.signal.lfilter (+ the clamp) / scipy.signal.filtfilt on this machine's host, same data, one process
  host_python_loop_ms_extrapolated   the reference-style Python loop over the samples of ONE row of 1 s, times rows x seconds: an
                             extrapolation, labelled as one
`rocprofv3 --kernel-trace --stats -- python tools/iir_filter_bench.py --once` is the run of its own for the kernel table.
No threshold: the figures are measurements."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0  # bench.py


def python_biquad_loop(x, b, a):
    """One row, the way the reference walks it: a Python loop over the samples."""
    out = np.empty_like(x)
    o1 = o2 = i1 = i2 = 0.0
    for j in range(x.shape[0]):
        o0 = x[j] * b[0] + i1 * b[1] + i2 * b[2] - o1 * a[1] - o2 * a[2]
        i2, i1, o2, o1 = i1, x[j], o1, o0
        out[j] = min(o0, 1.0)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--sample-rate", type=int, default=16000)
    ap.add_argument("--cutoff", type=float, default=1500.0)
    ap.add_argument("--chunks", type=int, nargs="+", default=[64, 128, 256, 512, 1024])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="warm up, run each function ONCE and exit (for a kernel trace)")
    a = ap.parse_args(argv)

    import scipy.signal
    import torch

    from mindaudio_amd import _lib
    from mindaudio_amd.data import filters as F

    rng = np.random.default_rng(0)
    x_np = (0.3 * (2.0 * rng.random((a.batch, a.samples)) - 1.0)).astype(np.float32)
    rows32 = torch.from_numpy(x_np).cuda()
    time_first = rows32.t().contiguous()  # (n, n_channel): what low_pass_filter takes
    result = {"batch": a.batch, "samples": a.samples, "sample_rate": a.sample_rate, "device": torch.cuda.get_device_name(0),
              "default_chunk": F.CHUNK}

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
        return start.elapsed_time(end) / iters

    b_lp, a_lp = F.low_pass_biquad(a.sample_rate, a.cutoff)
    a_lp1 = np.array([1.0, a_lp[1], a_lp[2]])
    b_ff, a_ff, zi_ff, padlen = F.filtfilt_design(4, 0.1, "lowpass")
    if a.once:
        for _ in range(a.warmup + 1):
            F.low_pass_filter(time_first, a.sample_rate, a.cutoff)
            F.filtfilt(rows32, 4, 0.1, "lowpass")
        torch.cuda.synchronize()
        return

    def kernel_table(rows, b, a1, **kw):
        table = {}
        out = torch.empty_like(rows)
        nbytes = 3 * rows.numel() * rows.element_size()
        for chunk in a.chunks:
            plan = F.iir_plan(b, a1, rows.shape[1], chunk=chunk)
            if plan.path != F.CHUNK_CARRY or plan.L != chunk:
                table[str(chunk)] = {"plan": "not usable: the plan gives L = %d (%s)" % (plan.L, plan.path)}
                continue
            call = lambda steps=0: F.iir_filter_device(rows, b, a1, out=out, plan=plan, _steps=steps, **kw)  # noqa: E731
            ms = timed(call)
            parts = [timed(lambda s=s: call(s)) for s in (_lib.IIR_STEP_CHUNK_STATES, _lib.IIR_STEP_CARRY, _lib.IIR_STEP_EMIT)]
            table[str(chunk)] = {
                "device_event_ms": round(ms, 4), "ms_chunk_states": round(parts[0], 4), "ms_carry": round(parts[1], 4),
                "ms_emit": round(parts[2], 4), "share_chunk_states_carry_emit": [round(p / sum(parts), 3) for p in parts],
                "must_move_mb": round(nbytes / 1e6, 2), "gb_per_s": round(nbytes / 1e9 / (ms * 1e-3), 1),
                "hbm_frac": round(nbytes / 1e9 / (ms * 1e-3) / HBM_PEAK_GBS, 4)}
        return table

    # ---- low_pass_filter ----
    ms = timed(lambda: F.low_pass_filter(time_first, a.sample_rate, a.cutoff))
    t0 = time.perf_counter()
    np.minimum(scipy.signal.lfilter(b_lp, a_lp1, x_np.astype(np.float64), axis=-1), 1.0).astype(np.float32)
    host_ms = (time.perf_counter() - t0) * 1e3
    one_second = x_np[0, :a.sample_rate].copy()
    t0 = time.perf_counter()
    python_biquad_loop(one_second, b_lp, a_lp)
    loop_ms = (time.perf_counter() - t0) * 1e3 * a.batch * a.samples / len(one_second)
    result["low_pass_filter"] = {"device_event_ms": round(ms, 4), "kernel": kernel_table(rows32, b_lp, a_lp1, upper_clamp=True),
                                 "host_scipy_ms": round(host_ms, 1), "host_python_loop_ms_extrapolated": round(loop_ms, 0)}
    # ---- filtfilt ----
    ms = timed(lambda: F.filtfilt(rows32, 4, 0.1, "lowpass"))
    ext = F.odd_extend(rows32.to(torch.float64), padlen)
    t0 = time.perf_counter()
    scipy.signal.filtfilt(b_ff, a_ff, x_np.astype(np.float64))
    host_ms = (time.perf_counter() - t0) * 1e3
    result["filtfilt_4_0.1_lowpass"] = {"device_event_ms": round(ms, 4), "padlen": padlen,
                                        "kernel": kernel_table(ext, b_ff, a_ff, zi=zi_ff, zi_mode="times-x0"),
                                        "host_scipy_ms": round(host_ms, 1)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
