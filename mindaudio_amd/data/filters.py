"""mindaudio.data.filters (filters.py): notch_filter, a host function, and the IIR family on the device - cal_filter_by_coffs (the
biquad recursion), its two designers low_pass_filter and peaking_equalizer, and filtfilt (scipy.signal.butter + scipy.signal.filtfilt).

The recursion runs in csrc/iir_filter.hip (ma_iir_filter, include/mindaudio_amd.h): the transposed direct form II of
scipy.signal.lfilter in float64, rows cut into chunks whose final states are carried by the chunk's transition matrix P = A^L.
`iir_plan` decides on the host whether that is sound for a filter; where it is not, every row is one sequential recursion.

One departure: the reference's cal_filter_by_coffs overwrites its argument and returns it; these functions leave their input alone
and return a new array or tensor.  contrast, riaa_biquad, treble_biquad and dcshift are MindSpore dataset ops in the reference and
are not built."""
import collections
import ctypes
import functools

import numpy as np

from .. import _host, _lib

__all__ = ["notch_filter", "cal_filter_by_coffs", "low_pass_filter", "peaking_equalizer", "filtfilt"]

CHUNK = 256  # samples a thread owns when carries are chained (DESIGN.md "IIR filters": the alternatives that were timed)
SEQUENTIAL, CHUNK_CARRY = "sequential", "chunk-carry"

IirPlan = collections.namedtuple("IirPlan", "L P path")


def notch_filter(notch_freq, filter_width=101, notch_width=0.05):
    """(1, filter_width, 1) float64 notch kernel: a low-pass below and a high-pass above `notch_freq` (a fraction of the Nyquist
    rate), Blackman-windowed sincs with the reference's constants (cutoff factor 3, `np.blackman(width + 1)[:-1]`)."""
    assert filter_width % 2 != 0
    assert 0 < notch_freq <= 1
    pad = filter_width // 2
    notch_freq += notch_width
    inputs = np.arange(filter_width) - pad

    def sinc(x):  # the zero is at the middle index
        return np.concatenate([np.sin(x[:pad]) / x[:pad], np.ones(1), np.sin(x[pad + 1:]) / x[pad + 1:]])

    window = np.blackman(filter_width + 1)[:-1]
    hlpf = sinc(3 * (notch_freq - notch_width) * inputs)
    hlpf *= window
    hlpf /= np.sum(hlpf)
    hhpf = sinc(3 * (notch_freq + notch_width) * inputs)
    hhpf *= window
    hhpf /= -np.sum(hhpf)
    hhpf[pad] += 1
    return (hlpf + hhpf).reshape(1, -1, 1)


# ---- IIR: the plan, the device call ----------------------------------------------------------------------------------------------------
def _normalised(b, a):
    b, a = np.atleast_1d(np.asarray(b, np.float64)), np.atleast_1d(np.asarray(a, np.float64))
    if b.ndim != 1 or a.ndim != 1 or a[0] == 0:
        raise ValueError("b and a must be one-dimensional with a[0] != 0")
    if a[0] != 1.0:
        b, a = b / a[0], a / a[0]
    n = max(len(a), len(b)) - 1
    return np.pad(b, (0, n + 1 - len(b))), np.pad(a, (0, n + 1 - len(a))), n


def transition_matrix(a):
    """A of the transposed direct form II with a[0] == 1: the state after one sample of zero input is A z
    (z_i' = z_(i+1) - a[i+1] z_0, because y = z_0)."""
    n = len(a) - 1
    A = np.zeros((n, n))
    A[:, 0] = -np.asarray(a, np.float64)[1:]
    A[np.arange(n - 1), np.arange(1, n)] = 1.0
    return A


CHUNK_LADDER = (1, 4, 16)  # multiples of `chunk` a plan tries, shortest first
POWER_TOLERANCE = 2.0 ** -44  # how far the two evaluations of P may be apart (absolute: a carried state is on the signal's scale)


@functools.lru_cache(maxsize=256)
def _carry_power(a_bytes, L):
    """P = np.linalg.matrix_power(A, L) if it can be trusted, else None.  Repeated squaring loses accuracy fast for a companion-like
    matrix with clustered poles (butter(8, 0.1): 20 % of P at L = 256, while every pole is inside the unit circle and P is finite),
    so P is checked against an independent evaluation, the product of L factors A taken one at a time - which is what the
    recursion itself does to a state over L samples of zero input."""
    A = transition_matrix(np.frombuffer(a_bytes, np.float64))
    with np.errstate(all="ignore"):
        P = np.linalg.matrix_power(A, L)
        if not np.all(np.isfinite(P)):
            return None
        Q = np.eye(len(A))
        for _ in range(L):
            Q = A @ Q
    if not np.all(np.isfinite(Q)) or np.abs(P - Q).max() > POWER_TOLERANCE:
        return None
    P.setflags(write=False)
    return P


def iir_plan(b, a, T, chunk=CHUNK, sequential=False):
    """Host only: how a filter runs over rows of T samples -> IirPlan(L, P, path).

    Chunk carry (P = np.linalg.matrix_power(A, L)) only when every pole np.roots(a) lies strictly inside the unit circle, P is
    finite and P agrees with the step-by-step product of L factors within POWER_TOLERANCE: then the carried states decay and the
    chunks compose as the sequential recursion does.  L is the first of chunk * CHUNK_LADDER that passes (a longer chunk has a
    smaller P, with a smaller error) and is shorter than T.  Otherwise - an unstable filter, or one whose transfer-function form is
    so ill-conditioned that no power of its transition matrix can be trusted, as scipy.signal.butter(8, 0.02, 'highpass') - one
    chunk per row: L = T, P = None, the plain sequential recursion in the reference's order, one thread per row.  Rows no longer
    than one chunk are one chunk either way.  `sequential=True` forces the second plan."""
    b, a, n = _normalised(b, a)
    T, chunk = int(T), int(chunk)
    if T < 1 or chunk < 1 or n < 1:
        raise ValueError("T, chunk and the filter order must be at least 1")
    if sequential or T <= chunk:
        return IirPlan(T, None, SEQUENTIAL)
    poles = np.roots(a)
    if not (np.all(np.isfinite(poles)) and np.all(np.abs(poles) < 1.0)):
        return IirPlan(T, None, SEQUENTIAL)
    for mult in CHUNK_LADDER:
        if chunk * mult >= T:
            break
        P = _carry_power(a.tobytes(), chunk * mult)
        if P is not None:
            return IirPlan(chunk * mult, P, CHUNK_CARRY)
    return IirPlan(T, None, SEQUENTIAL)


_ZI_MODES = {None: _lib.IIR_ZI_NONE, "as-is": _lib.IIR_ZI_AS_IS, "times-x0": _lib.IIR_ZI_TIMES_X0}


def iir_filter_device(rows, b, a, zi=None, zi_mode=None, reverse=False, upper_clamp=False, out=None, plan=None, _steps=0):
    """Device: (B, T) contiguous float32 / float64 rows through the order-n recursion of (b, a) -> a tensor of the same shape and
    dtype (`out`, which may be `rows`).  zi: n initial state values, used as they are (zi_mode "as-is") or times every row's first
    sample in processing order ("times-x0"); reverse: walk every row from its end; upper_clamp: store min(y, 1).  `plan`: an
    IirPlan, default iir_plan(b, a, T).  `_steps`: a mask of _lib.IIR_STEP_* for timing the launches one by one."""
    t = _host.require_gpu()
    b, a, n = _normalised(b, a)
    if n > _lib.IIR_MAX_ORDER:
        raise NotImplementedError("IIR filters up to order %d are built, got %d" % (_lib.IIR_MAX_ORDER, n))
    if rows.dim() != 2 or not rows.is_cuda or not rows.is_contiguous() or rows.dtype not in (t.float32, t.float64):
        raise ValueError("rows must be a contiguous (B, T) float32 or float64 device tensor")
    B, T = rows.shape
    if out is None:
        out = t.empty_like(rows)
    if B == 0 or T == 0:
        return out
    if plan is None:
        plan = iir_plan(b, a, T)
    if zi is not None and zi_mode is None:
        zi_mode = "as-is"
    zi_arr = None if zi is None else np.ascontiguousarray(zi, np.float64)
    if zi_arr is not None and zi_arr.shape != (n,):
        raise ValueError("zi must hold %d values" % n)
    P = None if plan.P is None else np.ascontiguousarray(plan.P, np.float64)
    if P is not None and P.shape != (n, n):
        raise ValueError("the plan's P must be (%d, %d)" % (n, n))
    host_ptr = lambda arr: None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    filt = _lib.IirFilter(n, _ZI_MODES[zi_mode if zi is not None else None], int(bool(reverse)), int(bool(upper_clamp)), int(plan.L),
                          host_ptr(b), host_ptr(a), host_ptr(zi_arr), host_ptr(P), int(_steps), 0)
    lib = _lib.load()
    nbytes = int(lib.ma_iir_filter_workspace_bytes(B, T, n, int(plan.L)))
    ws = _host.workspace(nbytes, rows.device) if nbytes else None
    rc = lib.ma_iir_filter(_host.ptr(rows), rows.element_size(), B, T, ctypes.byref(filt), _host.ptr(out),
                           _host.ptr(ws) if nbytes else None, nbytes, _host.current_stream_ptr())
    _lib.check(rc, "iir_filter")
    return out


def _floating_rows(x, what):
    """-> (device tensor float32 / float64 as given, was_numpy); TypeError for anything that is not floating point."""
    if isinstance(x, np.ndarray) or not hasattr(x, "is_cuda"):
        arr = np.asarray(x)
        if arr.dtype not in (np.float32, np.float64):
            raise TypeError("%s takes a float32 or float64 waveform, got %s" % (what, arr.dtype))
        t = _host.require_gpu()
        return t.from_numpy(np.ascontiguousarray(arr)).cuda(), True
    t = _host.torch()
    if x.dtype not in (t.float32, t.float64):
        raise TypeError("%s takes a float32 or float64 waveform, got %s" % (what, x.dtype))
    t = _host.require_gpu()
    return (x if x.is_cuda else x.cuda()), False


# ---- the biquads ---------------------------------------------------------------------------------------------------------------------------
def cal_filter_by_coffs(waveform, b, a):
    """filters.cal_filter_by_coffs: the biquad y[j] = b0 x[j] + b1 x[j-1] + b2 x[j-2] - a1 y[j-1] - a2 y[j-2] over `waveform` (n,) or
    (n, n_channel) - time first, channels interleaved - from a zero state.  As in the reference a[0] is never read (the designers
    leave their unnormalised a0 there), only b[0..2], a[1] and a[2] are; what is stored is min(y, 1.0) while the recursion goes on
    from the unclamped y, and nothing is clamped from below.  Arithmetic in float64, the result in the input's dtype.  NumPy in ->
    NumPy out, device tensor in -> device tensor out.  Unlike the reference the input is NOT overwritten: a new array is returned."""
    x, was_numpy = _floating_rows(waveform, "cal_filter_by_coffs")
    b, a = np.asarray(b, np.float64), np.asarray(a, np.float64)
    if b.shape != (3,) or a.shape != (3,):
        raise ValueError("b and a must hold three coefficients each")
    if x.dim() not in (1, 2):
        raise ValueError("waveform must be (n,) or (n, n_channel)")
    rows = x.reshape(1, -1) if x.dim() == 1 else x.t().contiguous()
    y = iir_filter_device(rows.contiguous(), b, np.array([1.0, a[1], a[2]]), upper_clamp=True)
    y = y.reshape(-1) if x.dim() == 1 else y.t().contiguous()
    return y.cpu().numpy() if was_numpy else y


def low_pass_biquad(sample_rate, cutoff_freq):
    """Host: (b, a) of filters.low_pass_filter - the cookbook low-pass at q = 0.707, b divided by a0, a = [a0, a1 / a0, a2 / a0]
    (a[0] is left unnormalised, as the reference leaves it)."""
    w0 = 2 * np.pi * cutoff_freq / sample_rate
    alpha = np.sin(w0) / (2 * 0.707)
    one_minus_cos = 1 - np.cos(w0)
    a0 = 1 + alpha
    return (np.array([one_minus_cos / 2 / a0, one_minus_cos / a0, one_minus_cos / 2 / a0]),
            np.array([a0, -2 * np.cos(w0) / a0, (1 - alpha) / a0]))


def peaking_biquad(sample_rate, center_freq, gain, q=0.707):
    """Host: (b, a) of filters.peaking_equalizer - the cookbook peaking filter with amplitude 10 ** (gain / 40), the same layout."""
    amp = np.exp(gain / 40 * np.log(10.0))
    w0 = 2 * np.pi * center_freq / sample_rate
    alpha = np.sin(w0) / (2 * q)
    a0 = 1 + alpha / amp
    minus_two_cos = -2 * np.cos(w0)
    return (np.array([(1 + alpha * amp) / a0, minus_two_cos / a0, (1 - alpha * amp) / a0]),
            np.array([a0, minus_two_cos / a0, (1 - alpha / amp) / a0]))


def low_pass_filter(waveform, sample_rate, cutoff_freq):
    """filters.low_pass_filter: the two-pole low-pass biquad at `cutoff_freq` Hz over (n,) or (n, n_channel); see cal_filter_by_coffs
    for the layout, the clamp and the types."""
    return cal_filter_by_coffs(waveform, *low_pass_biquad(sample_rate, cutoff_freq))


def peaking_equalizer(waveform, sample_rate, center_freq, gain, q=0.707):
    """filters.peaking_equalizer: the two-pole peaking biquad, `gain` dB at `center_freq` Hz; see cal_filter_by_coffs."""
    return cal_filter_by_coffs(waveform, *peaking_biquad(sample_rate, center_freq, gain, q))


# ---- filtfilt ------------------------------------------------------------------------------------------------------------------------------
def filtfilt_design(N, Wn, btype):
    """Host: what scipy.signal.filtfilt(b, a, x) works with for b, a = scipy.signal.butter(N, Wn, btype) and its defaults
    (padtype='odd') -> (b, a, zi, padlen): zi = scipy.signal.lfilter_zi(b, a), padlen = 3 * max(len(a), len(b))."""
    from scipy import signal

    b, a = signal.butter(N, Wn, btype)
    return b, a, signal.lfilter_zi(b, a), 3 * max(len(a), len(b))


def odd_extend(rows, padlen):
    """(B, T) -> (B, T + 2 padlen): scipy.signal's odd extension, 2 x[0] - x[padlen..1] in front and 2 x[-1] - x[-2..-padlen-1]
    behind (one rounding per sample, as SciPy's).  NumPy or tensor, T > padlen."""
    if isinstance(rows, np.ndarray):
        return np.concatenate([2 * rows[:, :1] - rows[:, padlen:0:-1], rows, 2 * rows[:, -1:] - rows[:, -2:-padlen - 2:-1]], axis=1)
    t = _host.torch()
    return t.cat([2 * rows[:, :1] - rows[:, 1:padlen + 1].flip(1), rows, 2 * rows[:, -1:] - rows[:, -padlen - 1:-1].flip(1)], dim=1)


def filtfilt_device(rows, b, a, zi, padlen, plan=None):
    """Device: (B, T) float64 rows -> (B, T) float64: odd extension, the forward pass from zi * x_ext[0], the backward pass (in
    place, walking every row from its end) from zi * y[last], the padding stripped.  Nothing is read back."""
    ext = odd_extend(rows, padlen)
    if plan is None:
        plan = iir_plan(b, a, ext.shape[1])
    y = iir_filter_device(ext, b, a, zi, "times-x0", plan=plan)
    y = iir_filter_device(y, b, a, zi, "times-x0", reverse=True, out=y, plan=plan)
    return y[:, padlen:-padlen].contiguous()


def filtfilt(waveform, N, Wn, btype, _sequential=False):
    """filters.filtfilt: a Butterworth filter of order N (band filters: 2 N) run forward and backward over the last axis of
    `waveform` (..., time), zero phase: scipy.signal.filtfilt(*scipy.signal.butter(N, Wn, btype), waveform) with SciPy's defaults.
    Both passes run in float64 whatever the input's type.  NumPy in -> float64 NumPy out, as SciPy's; device tensor in -> device
    tensor of the same dtype out.  ValueError when the time axis is not longer than padlen = 3 * (order + 1)."""
    b, a, zi, padlen = filtfilt_design(N, Wn, btype)
    shape = tuple(waveform.shape) if hasattr(waveform, "shape") else np.shape(waveform)
    if len(shape) < 1:
        raise ValueError("waveform must be (..., time)")
    if shape[-1] <= padlen:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
    x, was_numpy = _floating_rows(waveform, "filtfilt")
    t = _host.torch()
    rows = x.reshape(-1, shape[-1]).to(t.float64)
    plan = iir_plan(b, a, shape[-1] + 2 * padlen, sequential=_sequential)
    y = filtfilt_device(rows, b, a, zi, padlen, plan).reshape(shape)
    return y.cpu().numpy() if was_numpy else y.to(x.dtype)
