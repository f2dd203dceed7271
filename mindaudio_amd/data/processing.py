"""mindaudio.data.processing (processing.py) on MI355X through the C-ABI.

resample (the FFT method, resample.hip), unitarize and rescale (augment.hip), and - csrc/silence.hip - the silence front end trim /
split with their batched forms frame_power_device / trim_batch / split_batch, normalize (its float64 statistics from ma_axis_stats, applied by ma_axis_apply)
and stereo_to_mono (ma_channel_mean).  invert_channels, loop, clip and insert_in_background are indexing: NumPy in is answered in
NumPy, a device tensor with tensor ops, neither touches the other side.

NumPy in -> NumPy out, device tensor in -> device tensor out; no function overwrites its input (the reference's invert_channels
does: returning a new array is the one departure).  Quirks of the reference that are kept are named where they occur: trim's end
index is not clipped to the length, split clips with shape[-1] (the channel count of channel-last input), an all-zero signal is
non-silent throughout, invert_channels swaps the first and the last channel only.

Not built: sliding_window_cmn (a MindSpore dataset op in the reference; nothing executable pins it), overlap_and_add (works on
MindSpore tensors), resample's "minddata" method."""
import math

import numpy as np

from .. import _host, _lib

__all__ = ["resample", "resample_batch", "unitarize", "rescale", "normalize", "stereo_to_mono", "trim", "split", "invert_channels",
           "loop", "clip", "insert_in_background", "frame_power_device", "trim_batch", "split_batch"]


def resampled_length(n, orig_freq, new_freq):
    """n_samples of processing.py:164-166, with the reference's float arithmetic."""
    ratio = float(new_freq) / orig_freq
    return int(np.ceil(n * ratio))


def resample_batch(x, n_in, n_out, ni_dev=None, no_dev=None):
    """x (B, >= max(n_in)) float32 device tensor, n_in / n_out per-row lengths -> (B, max(n_out)) float32 with row b =
    scipy.signal.resample(x[b, :n_in[b]], n_out[b]) and zeros behind it.  ni_dev / no_dev: the same lengths as int32 device tensors
    when the caller has uploaded them already (the loader: no copy of its own behind a busy stream)."""
    t = _host.require_gpu()
    lib = _lib.load()
    assert x.is_cuda and x.dtype == t.float32 and x.dim() == 2 and x.stride(1) == 1
    n_in = np.asarray(n_in, np.int64)
    n_out = np.asarray(n_out, np.int64)
    b = x.shape[0]
    assert n_in.shape == (b,) and n_out.shape == (b,) and n_in.min() >= 1 and n_out.min() >= 1 and n_in.max() <= x.shape[1]
    max_in, max_out = int(n_in.max()), int(n_out.max())
    ws_bytes = lib.ma_resample_fft_workspace_bytes(b, max_in, max_out)
    _lib.check(min(ws_bytes, 0), "resample")
    ws = _host.workspace(ws_bytes, x.device)
    out = t.empty((b, max_out), dtype=t.float32, device=x.device)
    ni = ni_dev if ni_dev is not None else t.from_numpy(n_in.astype(np.int32)).to(x.device)
    no = no_dev if no_dev is not None else t.from_numpy(n_out.astype(np.int32)).to(x.device)
    rc = lib.ma_resample_fft_f32(_host.ptr(x), x.stride(0), _host.ptr(ni), _host.ptr(no), b, max_in, max_out, _host.ptr(out),
                                 out.stride(0), _host.ptr(ws), ws.numel(), _host.current_stream_ptr())
    _lib.check(rc, "resample")
    return out


def resample(waveform, orig_freq=16000, new_freq=16000, res_type="fft", lowpass_filter_width=6, rolloff=0.99, beta=None):
    """processing.resample: `[time]` or `[batch, time]`; res_type "fft" / "scipy" (scipy.signal.resample, processing.py:168-170).
    The "minddata" method goes through MindSpore's Resample in the reference and is not built."""
    if orig_freq == new_freq:
        return waveform  # processing.py:161-162
    if res_type not in ("scipy", "fft"):
        raise NotImplementedError("res_type %r uses MindSpore's Resample in the reference" % (res_type,))
    t = _host.require_gpu()
    was_numpy = not isinstance(waveform, t.Tensor)
    x = t.as_tensor(np.asarray(waveform) if was_numpy else waveform).to(device="cuda", dtype=t.float32)
    if x.dim() > 2:
        raise NotImplementedError("resample over [batch, time, channel] is not built")
    lead = tuple(x.shape[:-1])
    x2 = x.reshape((-1, x.shape[-1])).contiguous()
    n = x2.shape[-1]
    m = resampled_length(n, orig_freq, new_freq)
    y = resample_batch(x2, [n] * x2.shape[0], [m] * x2.shape[0]).reshape(lead + (m,))
    if was_numpy:
        return y.cpu().numpy().astype(np.asarray(waveform).dtype)  # np.asarray(y_hat, dtype=waveform.dtype), :170
    return y


def _unit(waveforms, lengths, amp_type, gain):
    """gain * waveforms / (amplitude + 1e-14) in one mix launch behind the row statistics."""
    from .. import ops
    from . import spectrum as _spectrum

    rows, restore, was_numpy = _spectrum._rows_channel_last(waveforms)
    t = _host.torch()
    stats = ops.aug_row_stats(rows)
    if amp_type == "avg":
        shape = tuple(np.shape(waveforms))
        lens = t.as_tensor(rows.shape[1] if lengths is None else lengths, dtype=t.float64).reshape(-1)
        if lens.numel() == 1:
            lens = lens.expand(rows.shape[0])
        elif len(shape) == 3:  # one length per batch entry, shared by its channels
            lens = lens.repeat_interleave(shape[2])
        params = t.zeros((rows.shape[0], 4), dtype=t.float64)
        params[:, 0] = lens
        out = ops.aug_mix(rows, _lib.AUG_MIX_UNIT_AVG, stats, gain=gain, params=params)
    else:
        out = ops.aug_mix(rows, _lib.AUG_MIX_UNIT_PEAK, stats, gain=gain)
    out = restore(out)
    return out.cpu().numpy() if was_numpy else out


def unitarize(waveforms, lengths=None, amp_type="avg", eps=1e-14):
    """processing.unitarize (processing.py:98-129): the waveforms over their average (sum |x| / lengths) or peak amplitude.
    `[time]`, `[batch, time]` or `[batch, time, channels]`; eps is the reference's 1e-14 (the kernel's constant)."""
    assert amp_type in ["avg", "peak"]
    if eps != 1e-14:
        raise NotImplementedError("eps other than the reference's default 1e-14 is not built")
    return _unit(waveforms, lengths, amp_type, 1.0)


def rescale(waveforms, target_lvl, lengths=None, amp_type="avg", dB=False):
    """processing.rescale (processing.py:189-232): unitarize, then scale to `target_lvl` (a scalar; in dB when dB=True).  As in the
    reference only amp_type="avg" passes both its own assertion ("max" | "avg") and unitarize's ("avg" | "peak")."""
    from .spectrum import dB_to_amplitude

    assert amp_type in ["max", "avg"]
    assert dB in [True, False]
    assert amp_type in ["avg", "peak"]  # unitarize's assertion, reached by the reference for "max"
    if np.ndim(target_lvl) != 0:
        raise NotImplementedError("rescale takes a scalar target level")
    gain = float(dB_to_amplitude(float(target_lvl), ref=1.0, power=0.5)) if dB else float(target_lvl)
    return _unit(waveforms, lengths, amp_type, gain)


# ---- shared marshalling ------------------------------------------------------------------------------------------------------------------
def _is_tensor(x):
    return hasattr(x, "is_cuda") and hasattr(x, "dtype") and not isinstance(x, np.ndarray)


def _on_device(x):
    """NumPy array-like or tensor -> (device tensor, was_numpy); needs a HIP device."""
    t = _host.require_gpu()
    if _is_tensor(x):
        return (x if x.is_cuda else x.cuda()), False
    return t.from_numpy(np.ascontiguousarray(np.asarray(x))).cuda(), True


def _back(y, was_numpy):
    return y.cpu().numpy() if was_numpy else y


def _is_complex(x):
    if _is_tensor(x):
        return x.is_complex()
    return np.issubdtype(np.asarray(x).dtype, np.complexfloating)


# ---- stereo_to_mono ------------------------------------------------------------------------------------------------------------------------
def _channel_mean_device(x):
    """(..., C) device tensor -> (...): ma_channel_mean in float32 / float64 (anything else is averaged in float64, as np.mean does)."""
    t = _host.torch()
    C = int(x.shape[-1])
    if C > _lib.CHANNEL_MEAN_MAX:
        raise NotImplementedError("stereo_to_mono is built for up to %d channels, got %d" % (_lib.CHANNEL_MEAN_MAX, C))
    if x.dtype not in (t.float32, t.float64):
        x = x.to(t.float64)
    x = x.contiguous()
    out = t.empty(tuple(x.shape[:-1]), dtype=x.dtype, device=x.device)
    if out.numel():
        rc = _lib.load().ma_channel_mean(_host.ptr(x), x.element_size(), out.numel(), C, _host.ptr(out), _host.current_stream_ptr())
        _lib.check(rc, "stereo_to_mono")
    return out


def stereo_to_mono(waveforms):
    """processing.stereo_to_mono: the mean over the last axis when ndim > 1 - (n, n_channel) -> (n,) - otherwise the input itself.
    The channels are added in the input's type in NumPy's order and divided by their count (csrc/silence.hip): float32 and float64
    results equal np.mean(waveforms, axis=-1) bit for bit.  Up to 8 channels; more raise NotImplementedError.  Complex input is not
    built."""
    ndim = waveforms.dim() if _is_tensor(waveforms) else np.ndim(waveforms)
    if ndim <= 1:
        return waveforms
    if _is_complex(waveforms):
        raise NotImplementedError("stereo_to_mono of complex input is not built")
    C = int(waveforms.shape[-1]) if hasattr(waveforms, "shape") else int(np.shape(waveforms)[-1])
    if C > _lib.CHANNEL_MEAN_MAX:
        raise NotImplementedError("stereo_to_mono is built for up to %d channels, got %d" % (_lib.CHANNEL_MEAN_MAX, C))
    if C < 1:
        raise ValueError("stereo_to_mono needs at least one channel")
    x, was_numpy = _on_device(waveforms)
    return _back(_channel_mean_device(x), was_numpy)


# ---- silence: frame power, trim, split ---------------------------------------------------------------------------------------------------
def num_frames(n, frame_length, hop_length):
    """Frames of a signal of n samples: the reference pads by frame_length // 2 on both sides and frames what it gets,
    (n + 2 * (frame_length // 2) - frame_length) // hop_length + 1 - n // hop_length + 1 for an even frame_length."""
    return (int(n) + 2 * (int(frame_length) // 2) - int(frame_length)) // int(hop_length) + 1


def _check_frames(frame_length, hop_length):
    if int(hop_length) < 1:
        raise ValueError("Invalid hop_length: {:d}".format(int(hop_length)))  # spectrum.frame, spectrum.py:295-296
    if int(frame_length) < 1:
        raise ValueError("Invalid frame_length: {:d}".format(int(frame_length)))
    return int(frame_length), int(hop_length)


def _device_lengths(lengths, B, T, device):
    """None, or B lengths as an int32 device tensor (a tensor is taken as it is: nothing is read back)."""
    if lengths is None:
        return None
    t = _host.torch()
    if _is_tensor(lengths):
        if tuple(lengths.shape) != (B,):
            raise ValueError("lengths must hold one entry per row")
        return lengths.to(device=device, dtype=t.int32).contiguous()
    arr = np.asarray(lengths, np.int64)
    if arr.shape != (B,) or arr.min() < 1 or arr.max() > T:
        raise ValueError("lengths must hold one entry per row, each in [1, T]")
    return t.from_numpy(arr.astype(np.int32)).to(device)


def _check_rows(rows):
    t = _host.torch()
    if not _is_tensor(rows) or rows.dim() != 2 or rows.dtype not in (t.float32, t.float64) or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError("rows must be a (B, T) float32 or float64 device tensor with B, T >= 1")
    t = _host.require_gpu()
    if not rows.is_cuda:
        raise ValueError("rows must live on the device")
    return rows if rows.stride(1) == 1 else rows.contiguous()


def frame_power_device(rows, lengths, frame_length, hop_length):
    """Device: rows (B, T) float32 / float64, lengths None or B entries (array or int32 device tensor) -> (power (B, Fmax) float64,
    row_max (B,) float64), Fmax = num_frames(T): power[b, f] = sqrt(mean(x^2))^2 of frame f of rows[b, :lengths[b]] zero-padded by
    frame_length // 2 on both sides, 0 behind the row's last frame.  Nothing is read back."""
    frame_length, hop_length = _check_frames(frame_length, hop_length)
    rows = _check_rows(rows)
    t = _host.torch()
    B, T = rows.shape
    lens = _device_lengths(lengths, B, T, rows.device)
    F = num_frames(T, frame_length, hop_length)
    power = t.empty((B, F), dtype=t.float64, device=rows.device)
    row_max = t.empty((B,), dtype=t.float64, device=rows.device)
    rc = _lib.load().ma_frame_power(_host.ptr(rows), rows.element_size(), B, T, rows.stride(0), None if lens is None else _host.ptr(lens),
                                    frame_length, hop_length, _host.ptr(power), F, _host.ptr(row_max), _host.current_stream_ptr())
    _lib.check(rc, "frame_power")
    return power, row_max


def _is_row_max(reference):
    return reference is None or reference is np.max or reference is np.amax or reference is max


def silence_edges_device(power, row_max, T, lens, frame_length, hop_length, top_db, reference, clip=-1):
    """Device: ma_silence_edges on frame_power_device's result -> (nonsilent (B, Fmax) uint8, trim_index (B, 2) int32, counts (B,)
    int32, edges (B, Fmax + 1) int32).  reference: None / np.max (the row maximum), a number, or a (B,) float64 device tensor."""
    t = _host.torch()
    B, F = power.shape
    ref_rows, ref_scalar = None, 0.0
    if _is_row_max(reference):
        ref_rows = row_max
    elif _is_tensor(reference):
        ref_rows = reference.to(device=power.device, dtype=t.float64).reshape(B).contiguous()
    else:
        ref_scalar = float(reference)
    flags = t.empty((B, F), dtype=t.uint8, device=power.device)
    index = t.empty((B, 2), dtype=t.int32, device=power.device)
    counts = t.empty((B,), dtype=t.int32, device=power.device)
    edges = t.empty((B, F + 1), dtype=t.int32, device=power.device)
    rc = _lib.load().ma_silence_edges(_host.ptr(power), F, B, T, None if lens is None else _host.ptr(lens), frame_length, hop_length,
                                      None if ref_rows is None else _host.ptr(ref_rows), ref_scalar, float(top_db), int(clip),
                                      _host.ptr(flags), _host.ptr(index), _host.ptr(counts), _host.ptr(edges),
                                      _host.current_stream_ptr())
    _lib.check(rc, "silence_edges")
    return flags, index, counts, edges


def _batch_edges(rows, lengths, top_db, reference, frame_length, hop_length):
    if reference is not None and not _is_row_max(reference) and not _is_tensor(reference) and callable(reference):
        raise NotImplementedError("the batched entries take the row maximum, a number or a (B,) tensor as reference")
    if not _is_row_max(reference) and not _is_tensor(reference):
        reference = float(np.abs(reference))  # amplitude_to_dB takes np.abs of a number
    frame_length, hop_length = _check_frames(frame_length, hop_length)
    rows = _check_rows(rows)
    lens = _device_lengths(lengths, rows.shape[0], rows.shape[1], rows.device)
    power, row_max = frame_power_device(rows, lens, frame_length, hop_length)
    return silence_edges_device(power, row_max, rows.shape[1], lens, frame_length, hop_length, top_db, reference)


def trim_batch(rows, lengths=None, top_db=60, reference=None, frame_length=2048, hop_length=512):
    """Device: rows (B, T) -> (B, 2) int32 device tensor, row b = trim's index for rows[b, :lengths[b]] (end not clipped), or
    (-1, -1) where trim would raise because no frame is non-silent.  reference: None / np.max (each row's maximum), a number, or a
    (B,) tensor.  Nothing is read back."""
    return _batch_edges(rows, lengths, top_db, reference, frame_length, hop_length)[1]


def split_batch(rows, lengths=None, top_db=60, reference=None, frame_length=2048, hop_length=512):
    """Device: rows (B, T) -> (counts (B,) int32, edges (B, Fmax + 1) int32): edges[b, :2 * counts[b]].reshape(-1, 2) = split's
    intervals for rows[b, :lengths[b]], clipped to lengths[b] (the time length), -1 behind them.  Nothing is read back."""
    return _batch_edges(rows, lengths, top_db, reference, frame_length, hop_length)[2:]


def host_edges(non_silent, hop_length):
    """Host, NumPy: the kernel's boundary logic on one row of flags -> (trim index (2,) or None, split edges before clipping).  A
    boundary is an index i in [0, F] where the flag changes, both ends counting as silent."""
    ns = np.concatenate([[False], np.asarray(non_silent, bool), [False]])
    bounds = np.flatnonzero(ns[1:] != ns[:-1]).astype(np.int64)
    if bounds.size == 0:
        return None, bounds
    return np.array([bounds[0], bounds[-1]], np.int64) * int(hop_length), bounds * int(hop_length)


def _single_edges(waveforms, top_db, reference, frame_length, hop_length, clip):
    frame_length, hop_length = _check_frames(frame_length, hop_length)
    shape = tuple(waveforms.shape) if hasattr(waveforms, "shape") else np.shape(waveforms)
    if len(shape) not in (1, 2) or shape[0] < 1:
        raise ValueError("waveforms must be (n,) or (n, n_channel) with n >= 1")
    if _is_complex(waveforms):
        raise NotImplementedError("complex waveforms are not built")
    if not _is_row_max(reference) and not callable(reference):
        reference = float(np.abs(reference))  # amplitude_to_dB takes np.abs of a number, and a callable's result as it is
    x, _ = _on_device(waveforms)
    t = _host.torch()
    mono = _channel_mean_device(x) if x.dim() > 1 else x
    if mono.dtype not in (t.float32, t.float64):
        mono = mono.to(t.float64)
    rows = mono.reshape(1, -1)
    power, row_max = frame_power_device(rows, None, frame_length, hop_length)
    if callable(reference) and not _is_row_max(reference):
        reference = float(reference(power[0].cpu().numpy()))  # any other callable: on the power row, on the host
    return silence_edges_device(power, row_max, rows.shape[1], None, frame_length, hop_length, top_db, reference, clip)


def trim(waveforms, top_db=60, reference=np.max, frame_length=2048, hop_length=512):
    """processing.trim: keep what lies between the first and the last non-silent frame of (n,) or (n, n_channel) -> (trimmed,
    index), index = np.array([start, end]) in samples and trimmed = waveforms[start:end].  A frame is non-silent when its power is
    within top_db decibels of `reference`: np.max / np.amax (the largest frame power, taken on the device), a number, or any other
    callable, which is called on the float64 power row read back to the host.
    Kept from the reference: end = (last non-silent frame + 1) * hop_length is NOT clipped to the length (its docstring example
    says 3000, its code and this return 3072); an all-zero signal is non-silent throughout (every frame sits at the 1e-10 floor, 0 dB
    from itself); and when no frame is non-silent (a number above every frame) it raises IndexError."""
    _, index, _, _ = _single_edges(waveforms, top_db, reference, frame_length, hop_length, -1)
    i0, i1 = (int(v) for v in index[0].cpu().numpy())
    if i0 < 0:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")  # edges[0][0] of the reference's empty edge list
    return waveforms[i0:i1], np.array([i0, i1])


def split(waveforms, top_db=60, reference=np.max, frame_length=2048, hop_length=512):
    """processing.split: the non-silent intervals of (n,) or (n, n_channel) as an (m, 2) NumPy int array of [start, end) in samples;
    `reference` as for trim.  Kept from the reference: the intervals are clipped with waveforms.shape[-1], which is the length for
    (n,) and the CHANNEL COUNT for channel-last input (split_batch clips to the time length); an all-zero signal is one interval; no
    non-silent frame gives an empty (0, 2) array."""
    shape = tuple(waveforms.shape) if hasattr(waveforms, "shape") else np.shape(waveforms)
    _, _, counts, edges = _single_edges(waveforms, top_db, reference, frame_length, hop_length, int(shape[-1]) if shape else -1)
    m = int(counts[0].cpu())
    return edges[0, :2 * m].cpu().numpy().astype(np.int64).reshape(-1, 2)


# ---- normalize ---------------------------------------------------------------------------------------------------------------------------
NORMS = ("max", "min", "mean", "mean_std", "l0", "l1", "l2")


def _axis_view(x, axis):
    """x (float32 / float64 / int32 / int64 after this, contiguous) viewed as (outer, n, inner) around `axis` (None: all of x) ->
    (x, dtype code, outer, n, inner, the statistics' shape with the axis kept)."""
    t = _host.torch()
    kinds = {t.float32: _lib.DTYPE_F32, t.float64: _lib.DTYPE_F64, t.int32: _lib.DTYPE_I32, t.int64: _lib.DTYPE_I64}
    if x.dtype not in kinds:
        if x.dtype.is_floating_point or x.dtype.is_complex:
            raise NotImplementedError("normalize is built for float32, float64 and integer input, got %s" % (x.dtype,))
        x = x.to(t.int64)
    x = x.contiguous()
    shape = tuple(x.shape)
    if axis is None:
        outer, n, inner, kept = 1, x.numel(), 1, (1,) * len(shape)
    else:
        outer, n, inner = math.prod(shape[:axis]), shape[axis], math.prod(shape[axis + 1:])
        kept = shape[:axis] + (1,) + shape[axis + 1:]
    if outer * n * inner == 0:
        raise ValueError("normalize of an empty array")
    return x, kinds[x.dtype], outer, n, inner, kept


def axis_stats_device(x, axis, stat):
    """Device: float64 statistic _lib.AXIS_* of |x| over `axis` (an int, or None for all of x) with the axis kept."""
    t = _host.torch()
    x, kind, outer, n, inner, kept = _axis_view(x, axis)
    out = t.empty((outer, inner), dtype=t.float64, device=x.device)
    rc = _lib.load().ma_axis_stats(_host.ptr(x), kind, outer, n, inner, int(stat), _host.ptr(out), _host.current_stream_ptr())
    _lib.check(rc, "normalize")
    return out.reshape(kept)


def axis_apply_device(x, axis, sub=None, div=None, as_float64=False):
    """Device: (x - sub) / div in float64 with the (axis-kept) statistics sub and div broadcast over `axis`, either left out; the
    result in x's dtype (rounded, or truncated toward zero for an integer) or, as_float64, in float64.  A new tensor."""
    t = _host.torch()
    x, kind, outer, n, inner, _ = _axis_view(x, axis)
    out = t.empty(x.shape, dtype=t.float64 if as_float64 else x.dtype, device=x.device)
    stat_ptr = lambda s: None if s is None else _host.ptr(s)  # noqa: E731
    sub, div = (None if s is None else s.to(t.float64).contiguous() for s in (sub, div))
    rc = _lib.load().ma_axis_apply(_host.ptr(x), kind, outer, n, inner, stat_ptr(sub), stat_ptr(div), _host.ptr(out),
                                   _lib.DTYPE_F64 if as_float64 else kind, _host.current_stream_ptr())
    _lib.check(rc, "normalize")
    return out


def normalize(waveforms, norm="max", axis=0):
    """processing.normalize: scale (or centre) an array along `axis` by a float64 statistic of its magnitude (csrc/silence.hip):
    "max", "min", "l0" (count of non-zeros), "l1", "l2" divide by it - a statistic below np.finfo(dtype).tiny (float32's for integer
    input) is replaced by 1 - and return the input's dtype, so integer input is truncated, as the reference's np.empty_like makes it;
    "mean" subtracts the mean and "mean_std" also divides by (std + 1e-5), both returning float64.  TypeError for an unknown norm,
    NotImplementedError for complex input."""
    if norm not in NORMS:
        raise TypeError("Unsupported norm type {}".format(repr(norm)))
    if _is_complex(waveforms):
        raise NotImplementedError("normalize of complex input is not built")
    ndim = waveforms.dim() if _is_tensor(waveforms) else np.ndim(waveforms)
    if axis is not None:
        if not isinstance(axis, (int, np.integer)):
            raise NotImplementedError("normalize takes one axis (an int) or None")
        if not -ndim <= axis < ndim:
            raise getattr(np, "exceptions", np).AxisError(int(axis), ndim)
        axis = int(axis) % ndim
    x, was_numpy = _on_device(waveforms)
    t = _host.torch()
    tiny = float(np.finfo({t.float32: np.float32, t.float64: np.float64}.get(x.dtype, np.float32)).tiny)
    if norm == "mean":
        return _back(axis_apply_device(x, axis, sub=axis_stats_device(x, axis, _lib.AXIS_MEAN), as_float64=True), was_numpy)
    if norm == "mean_std":
        mean, std = axis_stats_device(x, axis, _lib.AXIS_MEAN), axis_stats_device(x, axis, _lib.AXIS_STD)
        return _back(axis_apply_device(x, axis, sub=mean, div=std + 1e-5, as_float64=True), was_numpy)
    stat = {"max": _lib.AXIS_MAX, "min": _lib.AXIS_MIN, "l0": _lib.AXIS_L0, "l1": _lib.AXIS_SUM, "l2": _lib.AXIS_SUMSQ}[norm]
    scale = axis_stats_device(x, axis, stat)
    if norm == "l2":
        scale = scale.sqrt()
    scale = t.where(scale < tiny, t.ones_like(scale), scale)
    return _back(axis_apply_device(x, axis, div=scale).to(x.dtype), was_numpy)  # (int8 ... uint8 pass through the kernel as int64)


# ---- indexing: invert_channels, loop, clip, insert_in_background --------------------------------------------------------------------------
def invert_channels(waveform):
    """processing.invert_channels: (n, n_channel) with the FIRST and the LAST channel swapped - what the reference's code does,
    whatever its docstring says about reversing all of them; (n,) is returned as it is.  A new array: the reference swaps in place."""
    ndim = waveform.dim() if _is_tensor(waveform) else np.ndim(waveform)
    if ndim <= 1:
        return waveform
    out = waveform.clone() if _is_tensor(waveform) else np.array(waveform, copy=True)
    col = out.shape[1] - 1
    out[:, 0] = waveform[:, col]
    out[:, col] = waveform[:, 0]
    return out


def loop(waveform, times):
    """processing.loop: the signal repeated along its first axis, once per pass of the reference's `while times > 1` loop (so
    ceil(times) copies; the input itself for times <= 1)."""
    copies = 1
    while times > 1:
        copies += 1
        times -= 1
    if copies == 1:
        return waveform
    if _is_tensor(waveform):
        return _host.torch().cat([waveform] * copies, dim=0)
    return np.concatenate([np.asarray(waveform)] * copies, axis=0)


def clip(waveform, offset_factor, duration_factor):
    """processing.clip: waveform[int(offset * n):int((offset + duration) * n)] along the first axis; when offset + duration lies
    outside [0, 1] the reference prints and returns its input, and so does this."""
    if offset_factor + duration_factor < 0.0 or offset_factor + duration_factor > 1.0:
        print("Combination of offset and duration factors exceed audio length.")
        return waveform
    num_samples = waveform.shape[0]
    return waveform[int(offset_factor * num_samples):int((offset_factor + duration_factor) * num_samples), ...]


def insert_in_background(waveform, offset_factor, background_audio):
    """processing.insert_in_background: [background[:offset], waveform, background[:offset]] with offset = int(offset_factor *
    len(background)) - the reference repeats the HEAD of the background behind the signal, and so does this.  A background with
    another channel count is averaged to mono and tiled over the signal's channels.  offset_factor outside [0, 1]: prints, returns
    the input.  background_audio=None raises UnboundLocalError in the reference (num_channels is set in the other branch only):
    NotImplementedError here."""
    if offset_factor < 0.0 or offset_factor > 1.0:
        print("Offset factor number exceed range [0, 1].")
        return waveform
    if background_audio is None:
        raise NotImplementedError("background_audio=None: the reference's white-noise branch raises UnboundLocalError (its "
                                  "num_channels is assigned in the other branch only); pass a background")
    tensors = _is_tensor(waveform)
    if tensors != _is_tensor(background_audio):
        raise TypeError("waveform and background_audio must both be NumPy arrays or both be tensors")
    t = _host.torch() if tensors else None
    ndim = (lambda a: a.dim()) if tensors else np.ndim
    num_channels = 1 if ndim(waveform) == 1 else waveform.shape[1]
    bg_num_channels = 1 if ndim(background_audio) == 1 else background_audio.shape[1]
    if bg_num_channels != num_channels:
        if ndim(background_audio) > 1:
            background_audio = stereo_to_mono(background_audio) if tensors else np.mean(background_audio, axis=-1)
        if num_channels > 1:
            background_audio = (background_audio.unsqueeze(1).repeat(1, num_channels) if tensors
                                else np.tile(np.expand_dims(background_audio, axis=1), (1, num_channels)))
    offset = int(offset_factor * background_audio.shape[0])
    if num_channels > 1:
        parts = [background_audio[:offset, ...], waveform, background_audio[:offset, ...]]
        return t.cat(parts, dim=0) if tensors else np.vstack(parts)
    parts = [background_audio[..., :offset], waveform, background_audio[..., :offset]]
    return t.hstack(parts) if tensors else np.hstack(parts)
