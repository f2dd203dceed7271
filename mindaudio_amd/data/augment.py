"""Mirror of mindaudio.data.augment for the time-domain augmenters of ECAPA training-data generation (augment.py:101-792):
convolve1d, reverberate, add_reverb, add_noise, add_babble, drop_freq, drop_chunk, speed_perturb, rms_normalize, caculate_rms, on
MI355X through the kernels of csrc/augment.hip; and for its phase vocoder (augment.py:795-901): time_stretch, _phase_vocoder,
pitch_shift, through csrc/phase_vocoder.hip between the stft, istft and resample kernels.

Conventions, as everywhere in mindaudio_amd.data: NumPy in -> NumPy out, device tensor in -> device tensor out.  Arithmetic is
float32 on the device and the result is float32 - the reference returns float64 from most of these because it mixes in float64 file
data, and the example casts to float32 on its next line (train_speaker_embeddings.py:551).

Random decisions stay on the host and follow the reference's call order on the GLOBAL `np.random` and `random` generators: after
`np.random.seed(s); random.seed(s)` every function takes the reference's decisions and leaves both generators where the reference
leaves them.  Each function is split into a host part (`*_host`: draws, file reads, the composed notch filter, the rotated impulse
response, chunk intervals - small data) and a device part (`*_device`: rows in, rows out, nothing read back), which is what the
chain of ecapa/generate_train_data.py and the tests drive directly.

Deviations from the reference, on purpose:
  * reverberate on a 2-D array returns (B, T) with every row rescaled by its own amplitude; the reference returns (B, B, T) there,
    a broadcasting accident of `rescale` against a (B, 1, 1) amplitude.  (add_reverb never takes that path: it passes (B, T, 1).)
    A 1-D input comes back as (1, N), as from the reference.
  * rescale_amp: only "avg" can work in the reference ("peak" dies on an assertion of `rescale`, None on one of `unitarize`);
    anything else raises NotImplementedError here.
  * convolve1d: use_fft=True only (the other branch is a MindSpore Conv1d) and one kernel for the batch; `padding` as a tuple fails
    in the reference (`np.pad(..., pad=...)`) and raises here; an int is ignored, as there.
  * add_babble, drop_chunk and speed_perturb take `[batch, time]` (the shapes the example uses); `[batch, time, channels]` is not
    built for them.
  * _phase_vocoder accumulates the phase in float64 whatever the spectrogram's precision; the reference accumulates a complex64
    spectrogram's phase in float32 and rounds a growing phase at every step (DESIGN.md 8.2.1 has what that costs).  One rate per call.
Not built: frequencymasking, timemasking (MindSpore ops in the reference).
"""
import random

import numpy as np

from .. import _host, _lib, ops
from . import processing as _processing
from . import spectrum as _spectrum
from .filters import notch_filter
from .io import read
from .spectrum import _pad_shape, _rows_channel_last, dB_to_amplitude

__all__ = ["convolve1d", "reverberate", "add_reverb", "add_noise", "add_babble", "drop_freq", "drop_chunk", "speed_perturb",
           "rms_normalize", "caculate_rms", "time_stretch", "pitch_shift", "phase_vocoder_steps"]


def _rows_time_last(samples):
    """`[time]` / `[batch, time]` / `[batch, channels, time]` -> ((rows, time) float32 device rows, restore, was_numpy)."""
    t = _host.require_gpu()
    was_numpy = not isinstance(samples, t.Tensor)
    x = t.as_tensor(np.ascontiguousarray(samples) if was_numpy else samples).to(device="cuda", dtype=t.float32)
    if x.dim() == 0 or x.dim() > 3:
        raise NotImplementedError("samples must be [time], [batch, time] or [batch, channels, time]")
    lead = tuple(x.shape[:-1])
    return x.reshape(-1, x.shape[-1]), (lambda y: y.reshape(lead + (y.shape[-1],))), was_numpy


def _back(y, was_numpy):
    return y.cpu().numpy() if was_numpy else y


def _dev(a, device, dtype=None):
    t = _host.torch()
    a = np.ascontiguousarray(a, dtype=dtype)
    return t.from_numpy(a).to(device)


def _single_kernel(kernel, time_axis_last=False):
    """The one filter of a (K,), (1, K) or (1, K, 1) kernel as float64 (K,) - the batch shares it."""
    t = _host.torch()
    k = kernel.detach().cpu().numpy() if isinstance(kernel, t.Tensor) else np.asarray(kernel)
    if k.ndim > 3:
        raise NotImplementedError
    k = k.astype(np.float64)
    time_len = k.shape[0] if k.ndim == 1 else k.shape[1]
    if k.size != time_len:
        raise NotImplementedError("one kernel per batch entry or channel is not built: pass a single (K,), (1, K) or (1, K, 1) kernel")
    return k.reshape(-1)


# ---- convolution ---------------------------------------------------------------------------------------------------------------------
def rotated_kernel(kernel, n, rotation_index=0):
    """Host: what convolve1d(use_fft=True) makes of `kernel` for a signal of n samples - (taps float64 cut to n, rot) with the result
    y[i] = sum_k taps[k] x[(i + rot - k) mod n]  (kernel = concat(kernel[rot:], zeros, kernel[:rot]), circular convolution)."""
    taps = np.asarray(kernel, np.float64).reshape(-1)[:n]
    rot = int(rotation_index)
    if rot < 0:
        raise ValueError("rotation_index must not be negative")
    return taps, min(rot, taps.shape[0])


def convolve1d_device(rows, taps, rot=0, stats=None, out=None):
    """Device: circular convolution of every row with the host's (taps, rot); with `stats` rescaled to the rows' average amplitude."""
    return ops.aug_fft_conv(rows, _dev(taps, rows.device, np.float32), rot, stats, out)


def convolve1d(waveforms, kernel, padding=0, pad_type="constant", stride=1, groups=1, use_fft=True, rotation_index=0):
    """augment.convolve1d, use_fft=True: the circular convolution (no padding: the reference pads only for a tuple) of `[time]`,
    `[batch, time]` or `[batch, time, channels]` waveforms with one kernel, rolled by `rotation_index`."""
    if not use_fft:
        raise NotImplementedError("use_fft=False is a MindSpore Conv1d in the reference")
    if isinstance(padding, tuple):
        raise NotImplementedError("tuple padding fails in the reference (np.pad has no `pad` argument)")
    if np.ndim(waveforms) > 3:
        raise NotImplementedError
    taps, rot = rotated_kernel(_single_kernel(kernel), np.shape(waveforms)[0 if np.ndim(waveforms) == 1 else 1], rotation_index)
    rows, restore, was_numpy = _rows_channel_last(waveforms)
    return _back(restore(convolve1d_device(rows, taps, rot)), was_numpy)


def reverberate_host(rir_waveform, n):
    """Host: (taps, rot) of reverberate - the impulse response cut to n samples, rolled so that its largest |sample| (searched over the
    whole response, before the cut) lands on lag 0."""
    rir = _single_kernel(rir_waveform)
    return rotated_kernel(rir, n, int(np.argmax(np.abs(rir))))


def reverberate_device(rows, taps, rot, out=None):
    """Device: statistics, FFT convolution, rescale to the clean average amplitude - y / (amp(y) + 1e-14) * amp(x)."""
    return convolve1d_device(rows, taps, rot, ops.aug_row_stats(rows), out)


def reverberate(waveforms, rir_waveform, rescale_amp="avg"):
    """augment.reverberate: convolution with a room impulse response aligned on its direct path, at the clean signal's average
    amplitude.  `[time]` (returns (1, time), as the reference), `[batch, time]`, `[batch, time, channels]`."""
    if np.ndim(waveforms) > 3 or np.ndim(rir_waveform) > 3:
        raise NotImplementedError
    if rescale_amp != "avg":
        raise NotImplementedError("rescale_amp=%r cannot work in the reference (assertions of rescale / unitarize)" % (rescale_amp,))
    rows, restore, was_numpy = _rows_channel_last(waveforms)
    taps, rot = reverberate_host(rir_waveform, rows.shape[1])
    y = reverberate_device(rows, taps, rot)
    return _back(y if np.ndim(waveforms) == 1 else restore(y), was_numpy)


def add_reverb_host(rirlist, reverb_prob=1.0):
    """Host: the coin, then the file - None when the batch stays dry, else {"path", "rir"}."""
    if np.random.rand(1) > reverb_prob:
        return None
    path = random.choice(rirlist)
    rir, _ = read(path)
    return {"path": path, "rir": rir}


def add_reverb(samples, rirlist, reverb_prob=1.0):
    """augment.add_reverb: `[time]`, `[batch, time]` or `[batch, channels, time]` reverberated with one randomly chosen file."""
    if np.ndim(samples) > 3:
        if np.random.rand(1) > reverb_prob:  # (the reference draws before it looks at the shape)
            return samples
        raise NotImplementedError
    dec = add_reverb_host(rirlist, reverb_prob)
    if dec is None:
        return samples
    rows, restore, was_numpy = _rows_time_last(samples)
    taps, rot = reverberate_host(dec["rir"], rows.shape[1])
    return _back(restore(reverberate_device(rows, taps, rot)), was_numpy)


# ---- additive noise -------------------------------------------------------------------------------------------------------------------
def _rms_normalize_f64(samples):
    rms = np.sqrt(np.square(samples).mean(keepdims=True))
    return samples / (rms + 1e-8)


def add_noise_host(sample_length, backgroundlist, min_snr_in_db, max_snr_in_db, mix_prob=1.0):
    """Host: the coin, the file choices and the SNR.  None when nothing is mixed, else {"paths", "background" (float64, one row of
    sample_length: every piece rms-normalised on its own - a piece longer than what is missing is cut first - and the concatenation
    normalised again), "snr"}."""
    if np.random.rand(1) > mix_prob:
        return None
    missing = sample_length
    pieces, paths = None, []
    while missing > 0:
        path = random.choice(backgroundlist)
        paths.append(path)
        noise_audio, _ = read(path)
        if len(noise_audio) > missing:
            piece = _rms_normalize_f64(noise_audio[:missing])
            missing = 0
        else:
            piece = _rms_normalize_f64(noise_audio)
            missing -= len(noise_audio)
        pieces = piece if pieces is None else np.append(pieces, piece)
    background = _rms_normalize_f64(pieces.reshape(1, sample_length))[0]
    snr = np.random.uniform(min_snr_in_db, max_snr_in_db, 1)
    return {"paths": paths, "background": background, "snr": float(snr[0])}


def add_noise_device(rows, background, snr, out=None):
    """Device: rows + background * rms(row) / 10^(snr / 20); background: one float32 device row for the batch."""
    return ops.aug_mix(rows, _lib.AUG_MIX_NOISE, ops.aug_row_stats(rows), noise=background, gain=1.0 / (10.0 ** (snr / 20.0)), out=out)


def add_noise(samples, backgroundlist, min_snr_in_db, max_snr_in_db, mix_prob=1.0):
    """augment.add_noise: `[time]`, `[batch, time]` or `[batch, channels, time]`; ONE background row and ONE SNR for the batch."""
    if np.ndim(samples) > 3:
        if np.random.rand(1) > mix_prob:
            return samples
        raise NotImplementedError
    dec = add_noise_host(np.shape(samples)[-1], backgroundlist, min_snr_in_db, max_snr_in_db, mix_prob)
    if dec is None:
        return samples
    rows, restore, was_numpy = _rows_time_last(samples)
    y = add_noise_device(rows, _dev(dec["background"], rows.device, np.float32), dec["snr"])
    return _back(restore(y), was_numpy)


def rms_normalize(samples):
    """samples / (rms + 1e-8), the rms over ALL elements (augment.py:282-293)."""
    t = _host.require_gpu()
    was_numpy = not isinstance(samples, t.Tensor)
    x = t.as_tensor(np.ascontiguousarray(samples) if was_numpy else samples).to(device="cuda", dtype=t.float32)
    row = x.reshape(1, -1)
    y = ops.aug_mix(row, _lib.AUG_MIX_UNIT_RMS, ops.aug_row_stats(row)).reshape(x.shape)
    return _back(y, was_numpy)


def caculate_rms(samples):
    """sqrt(mean(x^2)) over the last axis (augment.py:296-307; the reference's spelling)."""
    rows, restore, was_numpy = _rows_time_last(samples)
    t = _host.torch()
    rms = t.sqrt(ops.aug_row_stats(rows)[:, 1] / rows.shape[1]).to(t.float32).reshape(tuple(np.shape(samples))[:-1])
    return _back(rms, was_numpy)


# ---- babble -----------------------------------------------------------------------------------------------------------------------------
def add_babble_host(lengths, n, speaker_count=3, snr_low=0, snr_high=0, mix_prob=1.0):
    """Host: the coin and one SNR per row.  None, or {"snr" (B, 1), "params" (B, 4) float64 = noise amplitude factor f =
    1 / (dB_to_amplitude(SNR, 1, 1) + 1) (the reference converts with power=1), the row's length and the babble's length in samples -
    the running maximum over the rolled rows, rolled as the reference rolls it}."""
    lens = np.expand_dims(np.asarray(lengths, np.float64) * n, axis=1)
    batch = lens.shape[0]
    if np.random.rand(1) > mix_prob:
        return None
    snr = np.random.rand(batch, 1)
    snr = snr * (snr_high - snr_low) + snr_low
    factor = 1 / (dB_to_amplitude(snr, 1, 1) + 1)
    babble_len = np.roll(lens, 1, axis=0)
    for _ in range(1, speaker_count):
        babble_len = np.maximum(babble_len, np.roll(babble_len, 1, axis=0))
    params = np.zeros((batch, 4), np.float64)
    params[:, 0], params[:, 1], params[:, 2] = factor[:, 0], lens[:, 0], babble_len[:, 0]
    return {"snr": snr, "params": params}


def add_babble_device(rows, params, speaker_count=3, out=None):
    """Device: babble = sum of the rows rolled by 1 .. speaker_count, out = (1 - f) x + f amp(x) / (amp(babble) + 1e-14) babble."""
    babble = ops.aug_babble_sum(rows, speaker_count)
    return ops.aug_mix(rows, _lib.AUG_MIX_BABBLE, ops.aug_row_stats(rows), noise=babble, params=_dev(params, rows.device, np.float64),
                       stats_noise=ops.aug_row_stats(babble), out=out)


def _rows_2d(waveforms, what):
    t = _host.require_gpu()
    if np.ndim(waveforms) != 2:
        raise NotImplementedError("%s takes [batch, time] waveforms" % what)
    was_numpy = not isinstance(waveforms, t.Tensor)
    x = t.as_tensor(np.ascontiguousarray(waveforms) if was_numpy else waveforms).to(device="cuda", dtype=t.float32)
    return x, was_numpy


def add_babble(waveforms, lengths, speaker_count=3, snr_low=0, snr_high=0, mix_prob=1.0):
    """augment.add_babble: every row mixed with the sum of the `speaker_count` rows before it in the batch; `lengths` are fractions
    of the time axis."""
    rows, was_numpy = _rows_2d(waveforms, "add_babble")
    if speaker_count < 1:
        raise ValueError("speaker_count must be at least 1")
    dec = add_babble_host(lengths.detach().cpu().numpy() if hasattr(lengths, "detach") else lengths, rows.shape[1], speaker_count,
                          snr_low, snr_high, mix_prob)
    if dec is None:
        return _back(rows.clone(), was_numpy)
    return _back(add_babble_device(rows, dec["params"], speaker_count), was_numpy)


# ---- drop_freq --------------------------------------------------------------------------------------------------------------------------
def compose_drop_filter(drop_frequency, drop_width=0.05, filter_length=101):
    """Host, float64: a delta at the middle index folded with each notch kernel by a CIRCULAR convolution of the filter's own length
    (what the reference's convolve1d does for an int padding)."""
    h = np.zeros(filter_length)
    h[filter_length // 2] = 1
    for frequency in drop_frequency:
        k = notch_filter(frequency, filter_length, drop_width).reshape(-1)
        h = np.fft.irfft(np.fft.rfft(h) * np.fft.rfft(k), n=filter_length)
    return h


def drop_freq_host(drop_freq_low=1e-14, drop_freq_high=1, drop_count_low=1, drop_count_high=2, drop_width=0.05, drop_prob=1):
    """Host: the coin, the count, the frequencies.  None, or {"drop_count", "drop_frequency", "filter" (101 float64 taps)}."""
    if np.random.rand(1) > drop_prob:
        return None
    drop_count = np.random.randint(low=drop_count_low, high=drop_count_high + 1, size=(1,))[0]
    drop_frequency = np.random.rand(drop_count) * (drop_freq_high - drop_freq_low) + drop_freq_low
    return {"drop_count": int(drop_count), "drop_frequency": drop_frequency, "filter": compose_drop_filter(drop_frequency, drop_width)}


def drop_freq_device(rows, drop_filter, out=None):
    """Device: y[i] = sum_k h[k] x[(i - k) mod n] - circular over the whole row and not centred (the output is delayed by the filter's
    half length and wraps), as the reference applies it; a filter longer than the row is cut to it."""
    taps = np.asarray(drop_filter, np.float64).reshape(-1)[:rows.shape[1]]
    return ops.aug_circular_fir(rows, _dev(taps, rows.device, np.float32), out)


def drop_freq(waveforms, drop_freq_low=1e-14, drop_freq_high=1, drop_count_low=1, drop_count_high=2, drop_width=0.05, drop_prob=1):
    """augment.drop_freq: notch filters at random frequencies (fractions of the Nyquist rate), one composed filter for the batch.
    `[time]`, `[batch, time]` or `[batch, time, channels]`."""
    rows, restore, was_numpy = _rows_channel_last(waveforms)
    dec = drop_freq_host(drop_freq_low, drop_freq_high, drop_count_low, drop_count_high, drop_width, drop_prob)
    if dec is None:
        return _back(restore(rows.clone()), was_numpy)
    return _back(restore(drop_freq_device(rows, dec["filter"])), was_numpy)


# ---- speed perturbation ------------------------------------------------------------------------------------------------------------------
def speed_perturb_host(n_speeds, perturb_prob=1.0):
    """Host: the coin and the index into `speeds`; None when the batch is left alone."""
    if np.random.rand(1) > perturb_prob:
        return None
    return int(np.random.randint(0, n_speeds, (1,))[0])


def speed_perturb_device(rows, orig_freq, speed):
    """Device: the rows resampled to orig_freq * speed // 100 (processing.resample); speed 100 returns the rows themselves."""
    return _processing.resample(rows, orig_freq, orig_freq * speed // 100)


def speed_perturb(waveform, orig_freq, speeds=[90, 100, 110], perturb_prob=1.0):
    """augment.speed_perturb: ONE speed for the batch, applied by resampling (`[time]` or `[batch, time]`)."""
    if np.ndim(waveform) > 2:
        raise NotImplementedError("speed_perturb over [batch, time, channels] is not built")
    idx = speed_perturb_host(len(speeds), perturb_prob)
    if idx is None:
        return waveform.copy() if isinstance(waveform, np.ndarray) else waveform.clone()
    new_freq = orig_freq * speeds[idx] // 100
    if new_freq == orig_freq:
        return waveform  # processing.resample hands the input back
    t = _host.require_gpu()
    if isinstance(waveform, t.Tensor):
        return _processing.resample(waveform.to(device="cuda", dtype=t.float32), orig_freq, new_freq)
    return _processing.resample(np.asarray(waveform, np.float32), orig_freq, new_freq)


# ---- drop_chunk ---------------------------------------------------------------------------------------------------------------------------
def drop_chunk_host(lengths, n, batch_size, drop_length_low=100, drop_length_high=1000, drop_count_low=1, drop_count_high=10,
                    drop_start=0, drop_end=None, drop_prob=1, noise_factor=0.0):
    """Host: validation, the coin, per row the count, then lengths, then starts (and, with noise, the uniform draws of every chunk), in
    the reference's order.  None, or {"drop_times", "length" / "start" (per row lists), "lens" (float64 lengths in samples),
    "intervals" int32 (B, n_max, 2) with Python's slice semantics applied, "fill" float32 / "fill_off" int32 (B, n_max) or None}."""
    if drop_length_low > drop_length_high:
        raise ValueError("Low limit must not be more than high limit")
    if drop_count_low > drop_count_high:
        raise ValueError("Low limit must not be more than high limit")
    if drop_end is not None and drop_end >= 0:
        if drop_start > drop_end:
            raise ValueError("Low limit must not be more than high limit")
        drop_range = drop_end - drop_start
        drop_length_low = min(drop_length_low, drop_range)
        drop_length_high = min(drop_length_high, drop_range)
    lens = np.asarray(lengths, np.float64) * n
    if np.random.rand(1) > drop_prob:
        return None
    drop_times = np.random.randint(low=drop_count_low, high=drop_count_high + 1, size=(batch_size,))
    n_max = int(drop_times.max()) if batch_size else 0
    intervals = np.zeros((batch_size, n_max, 2), np.int32)
    fill_off = np.zeros((batch_size, n_max), np.int32)
    fills, total = [], 0
    lengths_out, starts_out = [], []
    for i in range(batch_size):
        if drop_times[i] == 0:
            lengths_out.append(np.zeros(0, np.int64))
            starts_out.append(np.zeros(0, np.int64))
            continue
        length = np.random.randint(low=drop_length_low, high=drop_length_high + 1, size=(drop_times[i],))
        start_min = drop_start
        if start_min < 0:
            start_min += lens[i]
        start_max = drop_end
        if start_max is None:
            start_max = lens[i]
        if start_max < 0:
            start_max += lens[i]
        start_max = max(0, start_max - length.max())
        start = np.random.randint(low=start_min, high=start_max + 1, size=(drop_times[i],))
        end = start + length
        lengths_out.append(length)
        starts_out.append(start)
        for j in range(drop_times[i]):
            lo, hi, _ = slice(int(start[j]), int(end[j])).indices(n)
            intervals[i, j] = (lo, max(lo, hi))
            if noise_factor:
                if max(lo, hi) - lo != length[j]:
                    raise ValueError("could not broadcast input array from shape (%d,) into shape (%d,)" % (length[j], max(lo, hi) - lo))
                fills.append(np.random.rand(length[j]))
                fill_off[i, j] = total
                total += int(length[j])
    fill = np.concatenate(fills + [np.zeros(1)]).astype(np.float32) if noise_factor else None
    return {"drop_times": drop_times, "length": lengths_out, "start": starts_out, "lens": lens, "intervals": intervals, "fill": fill,
            "fill_off": fill_off if noise_factor else None}


def drop_chunk_device(rows, dec, noise_factor=0.0, out=None):
    """Device: the intervals zeroed, or filled with 2 m u - m (u the host's uniform draws, m = 2 noise_factor amp(row), the amplitude
    read from the statistics buffer); everything else copied bit for bit."""
    if dec["fill"] is None:
        return ops.aug_drop_chunks(rows, dec["intervals"], out=out)
    return ops.aug_drop_chunks(rows, dec["intervals"], _dev(dec["fill"], rows.device), dec["fill_off"], noise_factor,
                               ops.aug_row_stats(rows), _dev(dec["lens"], rows.device, np.float64), out=out)


def drop_chunk(waveforms, lengths, drop_length_low=100, drop_length_high=1000, drop_count_low=1, drop_count_high=10, drop_start=0,
               drop_end=None, drop_prob=1, noise_factor=0.0):
    """augment.drop_chunk: random chunks of every row set to zero (or to white noise scaled by the row's average amplitude);
    `lengths` are fractions of the time axis, chunks may overlap."""
    shape = tuple(np.shape(waveforms))
    if len(shape) != 2:
        if drop_length_low > drop_length_high or drop_count_low > drop_count_high:
            raise ValueError("Low limit must not be more than high limit")
        raise NotImplementedError("drop_chunk takes [batch, time] waveforms")
    lengths = lengths.detach().cpu().numpy() if hasattr(lengths, "detach") else lengths
    dec = drop_chunk_host(lengths, shape[1], shape[0], drop_length_low, drop_length_high, drop_count_low, drop_count_high, drop_start,
                          drop_end, drop_prob, noise_factor)
    rows, was_numpy = _rows_2d(waveforms, "drop_chunk")
    if dec is None:
        return _back(rows.clone(), was_numpy)
    return _back(drop_chunk_device(rows, dec, noise_factor), was_numpy)


# ---- phase vocoder: time_stretch, pitch_shift ------------------------------------------------------------------------------------------
def phase_vocoder_steps(frames, rate):
    """Host: the reference's time steps np.arange(0, frames, rate) (augment.py:841 - its own call, so the number of steps has its
    float quirks) as (int32 column index, float64 fraction np.mod(step, 1.0))."""
    steps = np.arange(0, frames, rate, dtype=np.float64)
    return steps.astype(np.int32), np.mod(steps, 1.0)


_step_tables = {}  # (frames, rate, device) -> the two tables on the device: they depend on shapes only, a repeated call uploads nothing


def _device_steps(frames, rate, device):
    key = (int(frames), float(rate), str(device))
    tables = _step_tables.get(key)
    if tables is None:
        if len(_step_tables) >= 64:
            _step_tables.clear()
        index, alpha = phase_vocoder_steps(frames, rate)
        tables = _step_tables[key] = (_dev(index, device, np.int32), _dev(alpha, device, np.float64))
    return tables


def phase_vocoder_device(spec, rate, hop_length):
    """Device: spec (B, n_freq, frames) complex64 -> (B, n_freq, steps) complex64, contiguous (what istft reads).  A transposed view
    of frame-major memory, as spectrum.stft returns, is read in place; anything else as bin-major rows."""
    t = _host.torch()
    b, n_freq, frames = spec.shape
    layout = _lib.STFT_FRAME_MAJOR
    if not spec.transpose(1, 2).is_contiguous():
        spec, layout = spec.contiguous(), _lib.STFT_FREQ_MAJOR
    index, alpha = _device_steps(frames, rate, spec.device)
    out = t.empty((b, n_freq, index.shape[0], 2), dtype=t.float32, device=spec.device)
    rc = _lib.load().ma_phase_vocoder_f32(_host.ptr(spec), layout, b, frames, n_freq, _host.ptr(index), _host.ptr(alpha), index.shape[0],
                                          int(hop_length), _host.ptr(out), _host.current_stream_ptr())
    _lib.check(rc, "_phase_vocoder")
    return t.view_as_complex(out)


def _phase_vocoder(matrix, rate, hop_length=None, n_fft=None):
    """augment._phase_vocoder: the spectrogram `matrix` (..., n_freq, frames) resampled along time at the steps 0, rate, 2 rate, ... -
    magnitudes interpolated between neighbouring columns, phases advanced by the accumulated wrapped phase difference.  NumPy in ->
    complex64 NumPy out, device tensor in -> device tensor out; what spectrum.stft returns for a tensor is taken without a copy."""
    if not rate > 0:
        raise ValueError("rate must be a positive number")
    t = _host.require_gpu()
    was_numpy = not isinstance(matrix, t.Tensor)
    D = t.as_tensor(np.asarray(matrix) if was_numpy else matrix).to(device="cuda", dtype=t.complex64)
    if D.dim() < 2:
        raise ValueError("matrix must be (..., 1 + n_fft/2, frames)")
    lead, n_freq, frames = tuple(D.shape[:-2]), D.shape[-2], D.shape[-1]
    if n_fft is None:
        n_fft = 2 * (n_freq - 1)
    if hop_length is None:
        hop_length = int(n_fft // 4)
    out = phase_vocoder_device(D.reshape((-1, n_freq, frames)), rate, hop_length)
    out = out.reshape(lead + tuple(out.shape[1:]))
    return out.cpu().numpy() if was_numpy else out


def time_stretch_device(rows, rate):
    """Device: (B, n) float32 rows -> (B, round(n / rate)) float32 - stft with its defaults, the vocoder on its frame-major memory,
    istft.  Nothing is read back."""
    spec = _spectrum.stft(rows)
    return _spectrum.istft(_phase_vocoder(spec, rate), length=int(round(rows.shape[-1] / rate)))


def time_stretch(waveforms, rate=None):
    """augment.time_stretch: `[time]`, `[batch, time]` (or more leading axes) made 1 / rate times as long without a change of pitch.
    NumPy in -> float64 NumPy out (the reference's istft buffer), device tensor in -> float32 device tensor out.  rate=None fails
    with the reference's TypeError."""
    if rate <= 0:
        raise ValueError("rate must be a positive number")
    rows, lead, was_numpy = _host.to_device_2d(waveforms)
    y = time_stretch_device(rows, rate)
    y = y.reshape(lead + (y.shape[-1],))
    return y.cpu().numpy().astype(np.float64) if was_numpy else y


def pitch_shift(waveforms, sr, n_steps, bins_per_octave=12):
    """augment.pitch_shift: time_stretch by rate = 2 ** (-n_steps / bins_per_octave), then resample from sr / rate back to sr.
    As in the reference the result is cut or zero-padded to the STRETCHED length round(n / rate), not to the input's n: the
    resampled signal has about n samples again and the rest is zeros (n_steps > 0) or a cut (n_steps < 0) - (2, 4000) at
    n_steps=4 comes back as (2, 5040).  NumPy in -> float64 NumPy out, device tensor in -> float32 device tensor out."""
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    rows, lead, was_numpy = _host.to_device_2d(waveforms)
    y = time_stretch_device(rows, rate)
    n = y.shape[-1]
    orig_freq = float(sr) / rate
    if orig_freq != sr:  # (processing.resample hands its input back otherwise)
        m = _processing.resampled_length(n, orig_freq, sr)
        y = _processing.resample_batch(y, [n] * y.shape[0], [m] * y.shape[0])
    y = _pad_shape(y, n)
    y = y.reshape(lead + (n,))
    return y.cpu().numpy().astype(np.float64) if was_numpy else y
