"""Drop-in mirrors of mindaudio.data.features on MI355X: fbank (features.py:196-270), mfcc, compute_deltas, context_window, and the
harmonic / percussive separation soft_mask, hpss and harmonic (features.py:438-559)."""
import math

import numpy as np

from .. import _host, _lib
from . import spectrum as _spectrum

__all__ = ["fbank", "fbanks", "mfcc", "compute_deltas", "context_window", "soft_mask", "hpss", "harmonic", "median_filter_device"]


def fbank(waveforms, deltas=False, context=False, n_mels=40, n_fft=400, sample_rate=16000, f_min=0.0, f_max=None,
          left_frames=5, right_frames=5, win_length=None, hop_length=None, window="hann"):
    """Filter-bank features: melspectrogram (power 2, centred, reflect pad, HTK mel) -> amplitude_to_dB
    (stype='power', ref=1.0, top_db=80.0), fused in one kernel (+ a tile-skipping floor pass).

    Shapes as the reference: [time] / [batch, time] / [batch, channel, time] ->
    [freq, time] / [batch, freq, time] / [batch, channel, freq, time].
    deltas/context (off in every in-tree call site) are outside the hot path.
    """
    if deltas or context:  # features.py:264-270: appended after the dB features
        out = fbank(waveforms, False, False, n_mels, n_fft, sample_rate, f_min, f_max, left_frames, right_frames,
                    win_length, hop_length, window)
        t_ = _host.require_gpu()
        was_np = not isinstance(out, t_.Tensor)
        od = t_.as_tensor(out).cuda() if was_np else out
        if deltas:
            d1 = compute_deltas(od)
            d2 = compute_deltas(d1)
            od = t_.cat((od, d1, d2), dim=-2)
        if context:
            od = context_window(od, left_frames, right_frames)
        return od.cpu().numpy() if was_np else od
    t = _host.require_gpu()
    lib = _lib.load()
    x, lead, was_numpy = _host.to_device_2d(waveforms)
    if len(lead) >= 2:
        # [batch, channel, time]: the top_db floor is per batch entry (spectrum.py:82-86) -> unfused path
        mel = _spectrum.melspectrogram(x.reshape(lead + (x.shape[-1],)), n_fft=n_fft, win_length=win_length,
                                       hop_length=hop_length, window=window, n_mels=n_mels,
                                       sample_rate=sample_rate, f_min=f_min, f_max=f_max)
        out = _spectrum.amplitude_to_dB(mel, stype="power", ref=1.0, top_db=80.0)
        return out.cpu().numpy() if was_numpy else out
    n = x.shape[-1]
    win_length, hop_length, win, bank = _spectrum._mel_args(n_fft, win_length, hop_length, window, True, "reflect",
                                                            n_mels, sample_rate, f_min, f_max, x.device)
    n_frames = lib.ma_num_frames(n, n_fft, hop_length, 1)
    _lib.check(min(n_frames, 0), "fbank")
    out = t.empty((x.shape[0], n_mels, n_frames), dtype=t.float32, device=x.device)
    ws_bytes = lib.ma_fbank_workspace_bytes(x.shape[0], n_frames)
    ws = _host.workspace(ws_bytes, x.device)
    amin, ref, top_db, mult = 1e-10, 1.0, 80.0, 10.0  # features.py:263 / spectrum.py:25
    rc = lib.ma_fbank_db_f32(_host.ptr(x), x.shape[0], n, x.stride(0), n_fft, hop_length, _host.ptr(win), 1,
                             _lib.PAD_MODES["reflect"], bank.ref(), 2.0, mult, amin,
                             mult * math.log10(max(amin, ref)), top_db, _host.ptr(out), _host.ptr(ws), ws.numel(),
                             _host.current_stream_ptr())
    _lib.check(rc, "fbank")
    out = out.reshape(lead + tuple(out.shape[1:]))
    return out.cpu().numpy() if was_numpy else out


fbanks = fbank  # README.md:41 and the docstring (features.py:247) spell it `fbanks`


# ---- post-processing of features.py -----------------------------------------------------------------
def _as_device_f32(x):
    t = _host.require_gpu()
    was_numpy = not isinstance(x, t.Tensor)
    xd = t.as_tensor(np.asarray(x) if was_numpy else x).to(device="cuda", dtype=t.float32).contiguous()
    return t, xd, was_numpy


def _back(out, was_numpy):
    return out.cpu().numpy() if was_numpy else out


def compute_deltas(specgram, win_length=5, pad_mode="edge"):
    """features.compute_deltas (features.py:158-193): delta coefficients along the last (time) axis."""
    if win_length < 3:
        raise ValueError("win_length must be no less than 3")
    t, x, was_numpy = _as_device_f32(specgram)
    out = t.empty_like(x)
    tlen = x.shape[-1]
    _lib.check(_lib.load().ma_compute_deltas_f32(_host.ptr(x), x.numel() // tlen, tlen, int(win_length),
                                                 _lib.PAD_MODES[pad_mode], _host.ptr(out), _host.current_stream_ptr()),
               "compute_deltas")
    return _back(out, was_numpy)


def context_window(waveforms, left_frames=0, right_frames=0):
    """features.context_window (features.py:64-155): [freq, time] / [batch, freq, time] / [batch, channel, freq, time]
    -> the same with freq * (left + right + 1) rows."""
    t, x, was_numpy = _as_device_f32(waveforms)
    shape = tuple(x.shape)
    if len(shape) not in (2, 3, 4):
        raise TypeError("Input dimension must be 2, 3 or 4, but got {}".format(len(shape)))
    f, tlen = shape[-2], shape[-1]
    batch = x.numel() // (f * tlen)
    cs = left_frames + right_frames + 1
    out = t.empty(shape[:-2] + (f * cs, tlen), dtype=t.float32, device=x.device)
    _lib.check(_lib.load().ma_context_window_f32(_host.ptr(x), batch, f, tlen, int(left_frames), int(right_frames),
                                                 _host.ptr(out), _host.current_stream_ptr()), "context_window")
    return _back(out, was_numpy)


def _create_dct(n_mfcc, n_mels, norm):
    """create_dct of mindspore.dataset.audio.utils (= torchaudio.functional.create_dct): (n_mels, n_mfcc) DCT-II."""
    n = np.arange(n_mels, dtype=np.float64)
    k = np.arange(n_mfcc, dtype=np.float64)[:, None]
    dct = np.cos(math.pi / n_mels * (n + 0.5) * k)
    if norm in (None, "none"):
        dct *= 2.0
    else:
        dct[0] *= 1.0 / math.sqrt(2.0)
        dct *= math.sqrt(2.0 / n_mels)
    return np.ascontiguousarray(dct.T).astype(np.float32)


def mfcc(waveforms, deltas=True, context=True, n_mels=23, n_mfcc=20, n_fft=400, sample_rate=16000, f_min=0.0, f_max=None,
         left_frames=5, right_frames=5, win_length=None, hop_length=None, norm="ortho", log_mels=False):
    """features.mfcc (features.py:273-373): melspectrogram -> dB (or log) -> DCT [-> deltas, delta-deltas] [-> context]."""
    if n_mfcc > n_mels:
        raise ValueError("The number of MFCC coefficients must be no more than # mel bins.")
    t = _host.require_gpu()
    was_numpy = not isinstance(waveforms, t.Tensor)
    mel = _spectrum.melspectrogram(waveforms if not was_numpy else t.as_tensor(np.asarray(waveforms)).cuda(),
                                   sample_rate=sample_rate, n_fft=n_fft, n_mels=n_mels, f_min=f_min, f_max=f_max,
                                   win_length=win_length, hop_length=hop_length)
    if log_mels:  # np.log(melspec + 1e-6), features.py:343-344
        mel = mel.contiguous()
        _lib.check(_lib.load().ma_pointwise_f32(_host.ptr(mel), mel.numel(), 1, 1e-6, 1.0, _host.ptr(mel),
                                                _host.current_stream_ptr()), "log mel")
    else:
        mel = _spectrum.amplitude_to_dB(mel, stype="power", ref=1.0, top_db=80.0)
    shape = tuple(mel.shape)
    tlen = shape[-1]
    batch = mel.numel() // (n_mels * tlen)
    dct = t.from_numpy(_create_dct(n_mfcc, n_mels, norm)).to(mel.device)
    out = t.empty(shape[:-2] + (n_mfcc, tlen), dtype=t.float32, device=mel.device)
    _lib.check(_lib.load().ma_dct_f32(_host.ptr(mel.contiguous()), batch, n_mels, tlen, _host.ptr(dct), n_mfcc, _host.ptr(out),
                                      _host.current_stream_ptr()), "mfcc dct")
    if deltas:
        d1 = compute_deltas(out)
        d2 = compute_deltas(d1)
        out = t.cat((out, d1, d2), dim=-2)
    if context:
        out = context_window(out, left_frames, right_frames)
    return _back(out, was_numpy)


# ---- harmonic / percussive separation (features.py:438-559; csrc/hpss.hip) ------------------------------------------------------------
MEDIAN_MAX_K = _lib.MEDIAN_MAX_K      # the widest median filter that is built
MEDIAN_SEGMENT = _lib.MEDIAN_SEGMENT  # outputs of a line that one workgroup stages (the tests put an axis on either side of it)


def _check_kernel(k, n, what):
    if int(k) != k:
        raise ValueError("%s kernel size must be an integer, got %r" % (what, k))
    if k < 1 or k > MEDIAN_MAX_K or k > 4 * n:
        raise ValueError("%s kernel size %d on an axis of %d: supported are 1 <= size <= %d and size <= 4 * axis length = %d (beyond "
                         "that scipy's reflect mode stops being the periodic reflection)" % (what, k, n, MEDIAN_MAX_K, 4 * n))
    return int(k)


def _float_dtype(t, dtype):
    return dtype if dtype in (t.float32, t.float64) else t.float32


def _dense_like(t, x):
    """(x or a contiguous copy of it, an uninitialised tensor of the same shape AND strides)"""
    out = t.empty_like(x)
    if out.stride() != x.stride():  # x is no dense permutation of its storage: the element-wise launches need one layout
        x = x.contiguous()
        out = t.empty_like(x)
    return x, out


def median_filter_device(x, size, axis=-1):
    """scipy.ndimage.median_filter(x, size=size along `axis` (-1 or -2) and 1 elsewhere, mode="reflect") of a float32 / float64
    device tensor (..., F, T), on the device: one launch, no copy for a dense tensor in either memory order (the frame-major view
    that stft returns included).  The result has x's strides and holds values of x, bit for bit."""
    t = _host.require_gpu()
    if axis not in (-1, -2) or x.dim() < 2:
        raise ValueError("median_filter_device filters the last or the last but one axis of a (..., F, T) tensor")
    k = _check_kernel(size, x.shape[axis], "median filter")
    if x.dtype not in (t.float32, t.float64) or not x.is_cuda:
        raise TypeError("median_filter_device takes a float32 or float64 device tensor")
    x, out = _dense_like(t, x)
    x3, o3 = x.reshape((-1,) + tuple(x.shape[-2:])), out.reshape((-1,) + tuple(x.shape[-2:]))
    if o3.data_ptr() != out.data_ptr() or o3.stride()[1:] != out.stride()[-2:]:
        raise AssertionError("a dense tensor's leading axes fold without a copy")
    other = -1 if axis == -2 else -2
    rc = _lib.load().ma_median_filter(_host.ptr(x3), _lib.DTYPE_F64 if x.dtype == t.float64 else _lib.DTYPE_F32, x3.shape[0],
                                      x3.shape[axis], x3.shape[other], x3.stride(0), x3.stride(axis), x3.stride(other), k,
                                      _host.ptr(o3), o3.stride(0), o3.stride(axis), o3.stride(other), _host.current_stream_ptr())
    _lib.check(rc, "median_filter")
    return out


def _soft_mask_launch(t, a, b, scale_b, power, split_zeros, want_mask, spec, phase, negative):
    """One ma_soft_mask launch on tensors of one layout -> the mask, or spec * mask (* phase)."""
    is_inf = math.isinf(power)
    res = None
    mask_p = spec_p = phase_p = out_p = None
    if want_mask:
        res = t.empty_like(a, dtype=t.bool if is_inf else a.dtype)
        mask_p = _host.ptr(res)
    else:
        res = t.empty_like(a, dtype=t.complex64 if phase is not None else a.dtype)
        spec_p, out_p = _host.ptr(spec), _host.ptr(res)
        phase_p = _host.ptr(phase) if phase is not None else None
    rc = _lib.load().ma_soft_mask(_host.ptr(a), _host.ptr(b), _lib.DTYPE_F64 if a.dtype == t.float64 else _lib.DTYPE_F32, a.numel(),
                                  1.0, float(scale_b), float(power), int(bool(split_zeros)), mask_p, spec_p, phase_p, out_p,
                                  _host.ptr(negative) if negative is not None else None, _host.current_stream_ptr())
    _lib.check(rc, "soft_mask")
    return res


_NEGATIVE = "x_input and x_ref must be non-negative"


def soft_mask(x_input, x_ref, *, power=1, split_zeros=False):
    """features.soft_mask (features.py:438-469): x_input ** power / (x_input ** power + x_ref ** power) with the reference's
    scaling by max(x_input, x_ref), 0 (or 0.5 with split_zeros) where both are below the type's tiny; power = inf gives the bool
    x_input > x_ref.  Any shape; float32 and float64 keep their type, everything else computes in float32.  NumPy in -> NumPy out,
    tensor in -> device tensor out.  Raises the reference's three TypeErrors (the shape and power ones before anything is
    launched; the non-negativity one reads back one flag the launch sets)."""
    x_shape, r_shape = tuple(np.shape(x_input)), tuple(np.shape(x_ref))
    if x_shape != r_shape:
        raise TypeError("x_input and x_ref shape mismatch.")
    if not power > 0:
        raise TypeError("power must be strictly positive.")
    t = _host.require_gpu()
    was_numpy = not isinstance(x_input, t.Tensor)
    a = t.as_tensor(np.ascontiguousarray(x_input) if was_numpy else x_input).cuda()
    b = t.as_tensor(np.ascontiguousarray(x_ref) if not isinstance(x_ref, t.Tensor) else x_ref).cuda()
    if a.is_complex() or b.is_complex():
        raise TypeError("soft_mask takes real input")
    dtype = _float_dtype(t, a.dtype)
    a, b = a.to(dtype).contiguous(), b.to(dtype).contiguous()
    if a.numel() == 0:
        return _back(t.empty_like(a, dtype=t.bool if math.isinf(power) else dtype), was_numpy)
    negative = t.zeros(1, dtype=t.int32, device=a.device)
    mask = _soft_mask_launch(t, a, b, 1.0, float(power), split_zeros, True, None, None, negative)
    if int(negative.item()):
        raise TypeError(_NEGATIVE)
    return _back(mask, was_numpy)


def _pair(value):
    return (value[0], value[1]) if not np.isscalar(value) else (value, value)


def hpss(spectrogram, *, kernel_size=31, power=2.0, mask=False, margin=1.0):
    """features.hpss (features.py:472-529): median-filter harmonic / percussive separation of a spectrogram (..., F, T), real
    (float32 / float64 keep their type, other real types compute in float32) or complex64 (magnitude and phase by magphase(power=1),
    the results complex64).  kernel_size and margin are a scalar or a (harmonic, percussive) pair; the harmonic filter runs along
    time, the percussive one along frequency, each scipy.ndimage.median_filter(mode="reflect") exactly (sizes up to 127 and up to
    four times the axis).  Returns (mask_harmonic, mask_percussive) with mask=True, else the two masked spectrograms.

    Four launches (two filters, one per output), no temporaries besides the two filtered arrays; a tensor input stays on the
    device and is never copied back - for real input the one "saw a negative value" flag is read, to raise the reference's
    TypeError.  The reference's magphase takes 2-D complex input only; leading axes are an extension here (every (F, T) slice is
    what the reference gives for it)."""
    margin_harmonic, margin_perc = _pair(margin)
    win_harmonic, win_perc = _pair(kernel_size)
    if margin_harmonic < 1 or margin_perc < 1:
        raise TypeError("Margins must be >= 1.0. A typical range is between 1 and 10.")
    if not power > 0:
        raise TypeError("power must be strictly positive.")
    shape = tuple(np.shape(spectrogram))
    if len(shape) < 2:
        raise ValueError("hpss takes a (..., F, T) spectrogram")
    win_harmonic = _check_kernel(win_harmonic, shape[-1], "harmonic (time)")
    win_perc = _check_kernel(win_perc, shape[-2], "percussive (frequency)")
    t = _host.require_gpu()
    was_numpy = not isinstance(spectrogram, t.Tensor)
    S = t.as_tensor(np.asarray(spectrogram) if was_numpy else spectrogram).cuda()
    phase = negative = None
    if S.is_complex():
        if S.dtype != t.complex64:
            raise NotImplementedError("hpss takes complex64 spectrograms (the reference's phase is complex64 too)")
        S, phase = _spectrum.magphase(S, power=1)  # contiguous float32 magnitude, complex64 phase
    else:
        S = S.to(_float_dtype(t, S.dtype))
        negative = t.zeros(1, dtype=t.int32, device=S.device)
    if S.numel() == 0:
        raise ValueError("hpss of an empty spectrogram")
    S, _ = _dense_like(t, S)
    harm = median_filter_device(S, win_harmonic, axis=-1)
    perc = median_filter_device(S, win_perc, axis=-2)
    split_zeros = margin_harmonic == 1 and margin_perc == 1
    ph = t.view_as_real(phase) if phase is not None and not mask else None
    out_h = _soft_mask_launch(t, harm, perc, margin_harmonic, float(power), split_zeros, mask, S, ph, negative)
    out_p = _soft_mask_launch(t, perc, harm, margin_perc, float(power), split_zeros, mask, S, ph, negative)
    if negative is not None and int(negative.item()):
        raise TypeError(_NEGATIVE)
    return _back(out_h, was_numpy), _back(out_p, was_numpy)


def harmonic(y_input, **kwargs):
    """features.harmonic (features.py:532-559): stft(n_fft=2048, pad_mode="constant") -> hpss(**kwargs)[0] -> istft(length=n), all
    on the device.  y_input (n,) or (..., n): every row is processed on its own and comes out as it would alone, bit for bit.  (The
    reference itself only runs for 1-D input - its magphase allocates a 2-D phase - so the batch is an extension.)  NumPy in ->
    float64 NumPy out, as the reference's istft returns; tensor in -> float32 device tensor out."""
    t = _host.require_gpu()
    was_numpy = not isinstance(y_input, t.Tensor)
    y = t.as_tensor(np.ascontiguousarray(y_input) if was_numpy else y_input).cuda()
    y_stft = _spectrum.stft(y, n_fft=2048, pad_mode="constant")
    stft_harm = hpss(y_stft, **kwargs)[0]
    # istft(stft_harm, length=n) with the frames inverted by the power-of-two FFT: ma_istft_f32's term-by-term sums at n_fft = 2048
    # round several times worse than everything else here
    y_harm = _spectrum._istft(stft_harm, None, None, None, "hann", True, y.shape[-1], True)
    return y_harm.cpu().numpy().astype(np.float64) if was_numpy else y_harm
