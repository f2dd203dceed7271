"""The cases of the IIR-filter fixtures, shared by tests/golden/gen_iir_goldens.py (which runs the reference's cal_filter_by_coffs,
low_pass_filter, peaking_equalizer and filtfilt on them) and test_iir_filter_cpu.py / test_iir_filter_gpu.py (which run ours).

golden/iir_goldens.npz holds, per case,
  x        the input: float32 for the biquads (what the reference is given - a copy, it overwrites its argument), float64 for filtfilt
  out      the reference's result on x (biquads: float32; filtfilt: float64)
  out64    biquads only: the reference's result on x held in a float64 array (nothing rounded on the way out)
  out32    filtfilt only: the reference's result on x rounded to float32 (float64, as SciPy returns it)
  e_in     [relative rms, max-abs over peak]: how far the reference's result moves when its input is rounded once to float32
  e_re     the same two figures for the spread between float64 evaluation orders: the largest difference from the reference's
           result over a direct-form-I loop, scipy.signal.lfilter and the NumPy chunk-carried evaluation below at chunks 64, 256
           and 1024 (those that stay finite and on the signal's scale)
  unclamped  the +12 dB case only: the recursion's output before min(y, 1)
No figure is measured on the code under test.  Every sample of every case is stored and compared: kept_samples is the identity.

The lengths follow the kernel's chunk length L = filters.CHUNK = 256 (and its ladder, 1024 for the filters whose P needs it): 1, 2, 3
(shorter than the state), L - 1, L, L + 1, 2 L, 3 L + 7 and 4 * 1024 + 7.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = os.path.join(HERE, "golden", "iir_goldens.npz")

L = 256  # mindaudio_amd.data.filters.CHUNK (test_iir_filter_cpu.py checks that it still is)
LONG = 4 * 1024 + 7
LENGTHS = (1, 2, 3, L - 1, L, L + 1, 2 * L, 3 * L + 7, LONG)


def noise(seed, shape, amp=0.3):
    """Seeded float64 noise, uniform in [-amp, amp): the generator's inputs (the fixtures store them, nothing depends on the stream
    staying what it is)."""
    return amp * (2.0 * np.random.default_rng(seed).random(shape) - 1.0)


# ---- biquads: name -> (function, arguments after the waveform, shape (time first), amplitude) -------------------------------------------
COFFS_B, COFFS_A = (0.2, 0.3, 0.1), (2.0, -0.5, 0.25)  # a[0] = 2 is never read
BIQUAD_CASES = {}
for _t in LENGTHS:
    BIQUAD_CASES["lp1500_%d" % _t] = ("low_pass_filter", (44100, 1500), (_t,), 0.3)
for _shape in ((3 * L + 7, 1), (3 * L + 7, 2), (3 * L + 7, 3)):
    BIQUAD_CASES["lp7000_ch%d" % _shape[1]] = ("low_pass_filter", (16000, 7000), _shape, 0.3)
BIQUAD_CASES["lp50_ch2"] = ("low_pass_filter", (16000, 50), (3 * 1024 + 7, 2), 0.3)  # P needs L = 1024
BIQUAD_CASES["peak_p12"] = ("peaking_equalizer", (44100, 1500, 12.0), (LONG,), 0.9)  # loud: crosses +1 and -1
BIQUAD_CASES["peak_m6_ch2"] = ("peaking_equalizer", (16000, 3000, -6.0, 2.0), (3 * L + 7, 2), 0.3)
BIQUAD_CASES["coffs"] = ("cal_filter_by_coffs", (np.array(COFFS_B), np.array(COFFS_A)), (4 * L + 7,), 0.3)
CLAMP_CASE = "peak_p12"

# ---- filtfilt: name -> ((N, Wn, btype), shape (time last)) -------------------------------------------------------------------------------
FILTFILT_CASES = {
    "lp2_min": ((2, 0.3, "lowpass"), (10,)),                    # T = padlen + 1
    "lp2_3d": ((2, 0.3, "lowpass"), (2, 3, 300)),               # 318 padded samples: two chunks
    "lp4_2d": ((4, 0.1, "lowpass"), (2, 1500)),
    "lp4_long": ((4, 0.1, "lowpass"), (LONG,)),
    "hp4": ((4, 0.05, "highpass"), (2600,)),                    # L = 1024
    "bp2": ((2, [0.1, 0.3], "bandpass"), (2, 500)),             # n = 4
    "bs3": ((3, [0.2, 0.5], "bandstop"), (700,)),               # n = 6
    "bp8": ((8, [0.2, 0.6], "bandpass"), (2, 600)),             # n = 16
    "hp8_seq": ((8, 0.02, "highpass"), (2, 800)),               # the reference docstring's filter: the sequential plan
}
SEQUENTIAL_CASES = ("hp8_seq",)


def case_seed(name):
    return sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % 100003


def kept_samples(n):
    """Every sample: the cases are small enough."""
    return np.arange(n)


def errors(y, ref, scale=None):
    """(relative rms, max-abs over peak) of y against ref, both relative to `scale` (default: ref itself); (0, 0) for two all-zero
    arrays."""
    ref = np.asarray(ref, np.float64)
    scale = ref if scale is None else np.asarray(scale, np.float64)
    err = np.abs(np.asarray(y, np.float64) - ref)
    rms, peak = np.sqrt(np.mean(scale ** 2)), np.abs(scale).max()
    return (float(np.sqrt(np.mean(err ** 2)) / rms) if rms > 0 else float(err.max()),
            float(err.max() / peak) if peak > 0 else float(err.max()))


# ---- float64 evaluations of the recursion in NumPy ----------------------------------------------------------------------------------------
def padded(b, a):
    b, a = np.asarray(b, np.float64), np.asarray(a, np.float64)
    n = max(len(a), len(b)) - 1
    return np.pad(b, (0, n + 1 - len(b))), np.pad(a, (0, n + 1 - len(a))), n


def transition(a):
    n = len(a) - 1
    A = np.zeros((n, n))
    A[:, 0] = -np.asarray(a)[1:]
    A[np.arange(n - 1), np.arange(1, n)] = 1.0
    return A


def tdf2(b, a, x, z):
    """The transposed direct form II over the last axis of x (..., S) from the states z (..., n) -> (y, final states); every leading
    index is an independent recursion."""
    b, a, n = padded(b, a)
    z = np.array(z, np.float64)
    y = np.empty(x.shape, np.float64)
    for s in range(x.shape[-1]):
        xs = x[..., s]
        ys = b[0] * xs + z[..., 0]
        y[..., s] = ys
        for i in range(n - 1):
            z[..., i] = b[i + 1] * xs + z[..., i + 1] - a[i + 1] * ys
        z[..., n - 1] = b[n] * xs - a[n] * ys
    return y, z


def chunked(b, a, x, L, P, zi=None, times_x0=False, reverse=False, upper_clamp=False):
    """The kernel's three steps in NumPy over rows x (B, T) in float64: every chunk of L samples from a zero state (the ragged last
    one carries nothing), z_(c+1) = P z_c + s_c, every chunk again from its true state.  P = None: one chunk per row."""
    b, a, n = padded(b, a)
    x = np.asarray(x, np.float64)
    if reverse:
        x = x[:, ::-1]
    B, T = x.shape
    z0 = np.zeros((B, n))
    if zi is not None:
        z0 = np.asarray(zi, np.float64)[None, :] * (x[:, :1] if times_x0 else np.ones((B, 1)))
    if P is None or T <= L:
        y, _ = tdf2(b, a, x, z0)
    else:
        C = -(-T // L)
        xc = np.pad(x, ((0, 0), (0, C * L - T))).reshape(B, C, L)
        _, s = tdf2(b, a, xc[:, :C - 1], np.zeros((B, C - 1, n)))
        z = np.empty((B, C, n))
        z[:, 0] = z0
        for c in range(C - 1):
            z[:, c + 1] = z[:, c] @ P.T + s[:, c]
        y, _ = tdf2(b, a, xc, z)
        y = y.reshape(B, C * L)[:, :T]
    if upper_clamp:
        y = np.minimum(y, 1.0)
    return y[:, ::-1] if reverse else y


def direct_form_1(b, a, x):
    """y[t] = sum_k b[k] x[t-k] - sum_k a[k] y[t-k] from rest over rows (B, T): the reference's own loop, at any order."""
    b, a, n = padded(b, a)
    B, T = x.shape
    xp, yp = np.concatenate([np.zeros((B, n)), x], 1), np.zeros((B, T + n))
    for t in range(T):
        acc = b[0] * xp[:, t + n]
        for k in range(1, n + 1):
            acc = acc + b[k] * xp[:, t + n - k]
        for k in range(1, n + 1):
            acc = acc - a[k] * yp[:, t + n - k]
        yp[:, t + n] = acc
    return yp[:, n:]


def odd_ext(x, padlen):
    return np.concatenate([2 * x[:, :1] - x[:, padlen:0:-1], x, 2 * x[:, -1:] - x[:, -2:-padlen - 2:-1]], axis=1)


def filtfilt_with(run, x, zi, padlen):
    """scipy.signal.filtfilt's order of operations over rows (B, T) with `run(rows, state (B, n)) -> rows` as its lfilter."""
    ext = odd_ext(x, padlen)
    y = run(ext, zi[None, :] * ext[:, :1])
    y = run(y[:, ::-1], zi[None, :] * y[:, -1:])[:, ::-1]
    return y[:, padlen:-padlen]
