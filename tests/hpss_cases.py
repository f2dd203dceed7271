"""The cases of the harmonic / percussive separation fixtures, shared by tests/golden/gen_hpss_goldens.py (which runs the reference's
soft_mask, hpss and harmonic of mindaudio/data/features.py on them) and test_hpss_cpu.py / test_hpss_gpu.py (which run ours).

golden/hpss_goldens.npz holds
  per real case      x (float32; only its sha256 where it has more than STORE_INPUT_MAX elements - the input is seeded), and per axis
                     and kernel size harm_off<k> / perc_off<k>: the reference's two scipy.ndimage.median_filter results, the generator having
                     recorded them inside the reference's hpss, stored as uint8 OFFSETS into each output's window (the first window
                     element that equals the result; a median filter's output is one of its window's inputs, so this loses
                     nothing: decode() gives the float32 array back, and the generator asserts that it does)
  per real run       (kernel size, power, margin): mask_h, mask_p (mask=True) and out_h, out_p (mask=False) of the reference's
                     hpss at the flat positions kept(shape)
  per soft_mask case a, b and the reference's mask
  per complex case   x (complex64, sha256 only) and per (margin): mask_h, mask_p, out_h, out_p at kept(shape)
  harmonic           x (6000 samples), the reference's float64 result and e32: (relative rms, max-abs over peak) between the
                     reference's harmonic as it stands (complex64 spectrogram) and the same code with the spectrogram kept
                     complex128
No figure is measured on the code under test.

Shapes.  The issue's four - (1025, 70), (33, 130), (3, 9, 12), (2, 2, 5, 8) - with its five kernel sizes wherever the size fits
(k <= 4 * axis), two that put an axis one below and one above the SEGMENT outputs of a line that a workgroup of csrc/hpss.hip
stages, a constant array, an all-zero one and one whose values come from four levels (ties everywhere).
"""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = os.path.join(HERE, "golden", "hpss_goldens.npz")

SEGMENT = 64  # MA_MEDIAN_SEGMENT (test_hpss_cpu.py checks that it still is)
MAX_K = 127   # MA_MEDIAN_MAX_K
STORE_INPUT_MAX = 8192
KERNELS = (31, 1, 4, (31, 17), (17, 20))


def case_seed(name):
    return sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % 100003


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pair(v):
    return (v, v) if np.isscalar(v) else (v[0], v[1])


def fits(kernel, shape):
    kh, kp = pair(kernel)
    return kh <= min(MAX_K, 4 * shape[-1]) and kp <= min(MAX_K, 4 * shape[-2])


def tag(v):
    return "x".join("%g" % p for p in pair(v))


# ---- the median filter's convention, written out ------------------------------------------------------------------------------------------
def reflect_index(j, n):
    """scipy's mode="reflect" as a periodic half-sample reflection: d c b a | a b c d | d c b a."""
    r = np.mod(j, 2 * n)
    return np.where(r < n, r, 2 * n - 1 - r)


def windows(x, k, axis):
    """(..., n, k) with the filtered axis moved last: output i's window, indices i - k // 2 ... i - k // 2 + k - 1 reflected."""
    x = np.moveaxis(x, axis, -1)
    n = x.shape[-1]
    return x[..., reflect_index(np.arange(n)[:, None] - k // 2 + np.arange(k)[None, :], n)]


def brute_median(x, k, axis):
    """The element of rank k // 2 of every sorted window."""
    return np.moveaxis(np.sort(windows(x, k, axis), axis=-1)[..., k // 2], -1, axis)


def encode(x, med, k, axis):
    w = windows(x, k, axis)
    hit = w == np.moveaxis(med, axis, -1)[..., None]
    assert hit.any(axis=-1).all(), "a median that is not in its window"
    return np.moveaxis(hit.argmax(axis=-1).astype(np.uint8), -1, axis)


def decode(x, off, k, axis):
    w = windows(x, k, axis)
    return np.moveaxis(np.take_along_axis(w, np.moveaxis(off, axis, -1)[..., None].astype(np.int64), axis=-1)[..., 0], -1, axis)


def kept(shape):
    """Flat positions of a result that the fixture stores: all of a small one, else every thirteenth (every forty-first of a
    large one) with both ends.  Both steps are odd: every residue of the kernels' 64-wide tiles is met."""
    size = int(np.prod(shape))
    if size <= 1024:
        return np.arange(size)
    return np.unique(np.concatenate([np.arange(0, size, 13 if size <= 16384 else 41), np.arange(8), np.arange(size - 8, size)]))


# ---- real spectrograms ------------------------------------------------------------------------------------------------------------------------
def mixture(seed, shape):
    """Seeded non-negative float32 (..., F, T): noise, a few horizontal lines (rows that stay loud over time: harmonic) and a few
    vertical ones (frames that are loud at every frequency: percussive), so that both masks take values across (0, 1)."""
    rng = np.random.default_rng(seed)
    F, T = shape[-2:]
    x = 0.2 * rng.random(shape)
    rows = rng.choice(F, size=max(1, F // 6), replace=False)
    cols = rng.choice(T, size=max(1, T // 6), replace=False)
    x[..., rows, :] += 0.5 + 0.5 * rng.random(shape[:-2] + (len(rows), T))
    x[..., :, cols] += 0.5 + 0.5 * rng.random(shape[:-2] + (F, len(cols)))
    return x.astype(np.float32)


REAL_CASES = {
    "big": dict(shape=(1025, 70), kind="mix", kernels=(31, (31, 17))),
    "mid": dict(shape=(33, 130), kind="mix", kernels=KERNELS),
    "b3": dict(shape=(3, 9, 12), kind="mix", kernels=KERNELS),
    "b22": dict(shape=(2, 2, 5, 8), kind="mix", kernels=tuple(k for k in KERNELS if fits(k, (5, 8)))),
    "seg_lo_hi": dict(shape=(SEGMENT - 1, SEGMENT + 1), kind="mix", kernels=(31,)),
    "seg_hi_lo": dict(shape=(SEGMENT + 1, SEGMENT - 1), kind="mix", kernels=(31,)),
    "const": dict(shape=(9, 12), kind="const", kernels=(31, 4)),
    "zeros": dict(shape=(9, 12), kind="zeros", kernels=(31, 4)),
    "ties": dict(shape=(33, 130), kind="ties", kernels=(31, 4)),
}
MULTI_REFLECTION = ("b22", (17, 20))  # 20 taps on an axis of 5: the window crosses more than one reflection


def real_input(name):
    c = REAL_CASES[name]
    if c["kind"] == "const":
        return np.full(c["shape"], 0.37, np.float32)
    if c["kind"] == "zeros":
        return np.zeros(c["shape"], np.float32)
    if c["kind"] == "ties":
        return np.random.default_rng(case_seed(name)).choice(np.array([0.0, 0.25, 0.5, 1.0], np.float32), size=c["shape"])
    return mixture(case_seed(name), c["shape"])


def real_runs(name):
    """(kernel, power, margin): every kernel size at the defaults; the first one also with power 1 and with margins (2, 4), except
    for the large case (the fixture file has a size to keep)."""
    c = REAL_CASES[name]
    ks = c["kernels"]
    more = [(ks[0], 1, 1.0), (ks[0], 2.0, (2.0, 4.0))] if int(np.prod(c["shape"])) <= STORE_INPUT_MAX else []
    return [(k, 2.0, 1.0) for k in ks] + more


def median_keys(name, kernel):
    """(harmonic: along time, percussive: along frequency) - one entry per axis and size, whatever pairs they occur in"""
    kh, kp = pair(kernel)
    return "real/%s/harm_off%d" % (name, kh), "real/%s/perc_off%d" % (name, kp)


def run_key(name, kernel, power, margin):
    return "real/%s/k%s/p%g/m%s" % (name, tag(kernel), power, tag(margin))


# ---- soft_mask --------------------------------------------------------------------------------------------------------------------------------
POWERS = (1, 2, 0.5, 3.7, np.inf)
EXACT_POWERS = (1, 2, np.inf)  # a copy, a product, a comparison: bit for bit; the others go through pow / sqrt: 4 eps
SOFT_DTYPES = ("float32", "float64")


def soft_mask_inputs(dtype):
    """(a, b) of shape (6, 40): seeded values in [0, 1), then exact zeros on either side and on both, values below the type's tiny
    on either side and on both (the `bad` branch needs both below it), tiny itself, and equal values."""
    rng = np.random.default_rng(case_seed("soft_" + dtype))
    a, b = rng.random((6, 40)), rng.random((6, 40))
    tiny = float(np.finfo(dtype).tiny)
    a[0, :8], b[0, :8] = 0.0, rng.random(8)
    a[1, :8], b[1, :8] = rng.random(8), 0.0
    a[2, :8] = b[2, :8] = 0.0
    a[3, :8], b[3, :8] = tiny * np.array([0.5, 0.25, 0.5, 0.0, 1.0, 2.0, 0.5, 0.75]), tiny * np.array([0.25, 0.5, 0.5, 0.5, 0.5, 0.5, 4.0, 0.75])
    a[4, :8], b[4, :8] = tiny * 0.5, rng.random(8)
    a[5, :8] = b[5, :8] = rng.random(8)
    return a.astype(dtype), b.astype(dtype)


def soft_key(dtype, power, split_zeros):
    return "soft/%s/p%g/s%d" % (dtype, power, int(split_zeros))


# ---- complex spectrograms -----------------------------------------------------------------------------------------------------------------------
COMPLEX_SHAPE = (257, 40)
COMPLEX_SLICES = ("c0", "c1")  # the (2, 257, 40) batch is these two; "c0" is the 2-D case
COMPLEX_MARGINS = (1.0, (2.0, 4.0))
MAG_FLOOR = 1e-6  # the generator asserts every magnitude is exactly zero or at least this: nothing sits at the `tiny` switch


def complex_input(name):
    rng = np.random.default_rng(case_seed(name))
    mag = mixture(case_seed(name) + 1, COMPLEX_SHAPE).astype(np.float64)
    mag[rng.random(COMPLEX_SHAPE) < 0.01] = 0.0  # a few exact zeros: phase 1 + 0j
    return (mag * np.exp(2j * np.pi * rng.random(COMPLEX_SHAPE))).astype(np.complex64)


def complex_key(name, margin):
    return "complex/%s/m%s" % (name, tag(margin))


# ---- harmonic -----------------------------------------------------------------------------------------------------------------------------------
HARMONIC_N = 6000  # the shortest with several frames at n_fft = 2048, hop 512


def harmonic_input(seed_name="harmonic"):
    """A few steady tones (harmonic), a few clicks (percussive) and noise."""
    rng = np.random.default_rng(case_seed(seed_name))
    t = np.arange(HARMONIC_N) / 16000.0
    y = 0.02 * rng.standard_normal(HARMONIC_N)
    for f in (220.0, 440.0, 1330.0):
        y += 0.2 * np.sin(2 * np.pi * f * t + rng.random() * 6.28)
    for pos in (700, 2500, 4100):
        y[pos:pos + 24] += 0.8 * rng.standard_normal(24)
    return y.astype(np.float32)


def errors(y, ref):
    """(relative rms, max-abs over peak): the yardstick of test_augment_gpu.py."""
    ref = np.asarray(ref, np.float64)
    err = np.asarray(y, np.float64) - ref
    return float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(ref ** 2))), float(np.abs(err).max() / np.abs(ref).max())
