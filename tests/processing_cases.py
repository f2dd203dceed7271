"""The cases of the data.processing fixtures, shared by tests/golden/gen_processing_goldens.py (which runs the reference's trim, split,
normalize, stereo_to_mono, invert_channels, loop, clip and insert_in_background on them) and test_processing_cpu.py /
test_processing_gpu.py (which run ours).

golden/processing_goldens.npz holds
  per silence case   x (float32, or float64 where the case says so), power (the reference's np.sqrt(power) ** 2 row), db (its
                     amplitude_to_dB row), flags (db > -top_db), margin (the smallest |db + top_db| over the frames: the generator
                     asserts it is at least MARGIN_DB), trim_index or trim_error (the exception's type name), split
  per normalize case x (float64; the float32 and int64 inputs are cast(x, dtype)), and per (norm, axis, dtype) the reference's
                     result at the flat positions kept(shape), plus for the summed statistics `spread`: the largest difference,
                     over the peak, between the reference run with NumPy's own summation, a reversed one and math.fsum
  per channel case   x, out;  per indexing case the arguments and the result
No figure is measured on the code under test.

The silence lengths follow the frame tiling of csrc/silence.hip (TILE frames per workgroup): 1, hop - 1, hop, hop + 1,
frame_length - 1, frame_length, 3 frame_length + 7, and the length that has TILE + 1 frames.  The (frame_length, hop_length) pairs
are the issue's six plus the two on either side of the kernel's hop-block threshold (ratio 32: block sums, ratio 33: direct sums).
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = os.path.join(HERE, "golden", "processing_goldens.npz")

TILE = 16       # MA_FRAME_POWER_TILE (test_processing_cpu.py checks that it still is)
MAX_RATIO = 32  # MA_FRAME_POWER_MAX_RATIO
MARGIN_DB = 1e-6
QUIET, LOUD = 1e-4, 0.3

PAIRS = ((2048, 512), (400, 160), (64, 16), (7, 3), (512, 512), (16, 40), (64, 2), (66, 2))


def case_seed(name):
    return sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % 100003


def num_frames(n, frame_length, hop_length):
    return (n + 2 * (frame_length // 2) - frame_length) // hop_length + 1


def sweep_lengths(frame_length, hop_length):
    cross = next(n for n in range(1, (TILE + 2) * hop_length + 2) if num_frames(n, frame_length, hop_length) == TILE + 1)
    cand = (1, hop_length - 1, hop_length, hop_length + 1, frame_length - 1, frame_length, 3 * frame_length + 7, cross)
    return tuple(dict.fromkeys(n for n in cand if n >= 1))


def blocks(seed, shape, block, phase):
    """Seeded float64 noise, uniform in [-level, level), whose level switches between LOUD and QUIET every `block` samples along the
    first axis; block k is loud when k + phase is even."""
    x = 2.0 * np.random.default_rng(seed).random(shape) - 1.0
    level = np.where((np.arange(shape[0]) // block + phase) % 2 == 0, LOUD, QUIET)
    return x * level.reshape((-1,) + (1,) * (len(shape) - 1))


# name -> dict(signal, shape, dtype, frame_length, hop_length, top_db, reference ("max" or a number)[, phase])
SILENCE_CASES = {}


def _add(name, signal, shape, dtype, fl, hop, top_db, reference="max", phase=None):
    SILENCE_CASES[name] = dict(signal=signal, shape=tuple(shape), dtype=dtype, frame_length=fl, hop_length=hop, top_db=top_db,
                               reference=reference, phase=case_seed(name) % 2 if phase is None else phase)


for _fl, _hop in PAIRS:
    for _n in sweep_lengths(_fl, _hop):
        _add("sw_%d_%d_%d" % (_fl, _hop, _n), "blocks", (_n,), "float32", _fl, _hop, 60)
_add("doc_trim", "doc_trim", (3000,), "float64", 2048, 512, 10)
_add("doc_split", "doc_split", (8192,), "float64", 2048, 512, 10)
_add("zeros", "zeros", (199,), "float32", 64, 16, 60)
_add("zeros_ch2", "zeros", (199, 2), "float64", 64, 16, 10)
for _fl, _hop in ((64, 16), (400, 160)):
    _n = (5 if _fl == 64 else 3) * (_fl + _hop)  # loud-quiet-loud(-quiet-loud) or the opposite
    for _db in (10, 60):
        _add("loud_ends_%d_%d" % (_fl, _db), "blocks", (_n,), "float32", _fl, _hop, _db, phase=0)
        _add("quiet_ends_%d_%d" % (_fl, _db), "blocks", (_n,), "float32", _fl, _hop, _db, phase=1)
    _add("f64_%d" % _fl, "blocks", (_n,), "float64", _fl, _hop, 60, phase=1)
for _c in (1, 2, 3):
    for _dt in ("float32", "float64"):
        _add("ch%d_%s" % (_c, _dt), "blocks", (400, _c), _dt, 64, 16, 60 if _c != 2 else 10, phase=1)
_add("ref_1_60", "blocks", (400,), "float32", 64, 16, 60, reference=1.0, phase=1)
_add("ref_001_10", "blocks", (400,), "float32", 64, 16, 10, reference=0.01, phase=0)
_add("ref_none_pass", "blocks", (400,), "float32", 64, 16, 10, reference=100.0, phase=0)
NONE_PASS_CASE = "ref_none_pass"


def silence_signal(name):
    c = SILENCE_CASES[name]
    if c["signal"] == "doc_trim":
        x = np.array([0.01] * 1000 + [0.6] * 1000 + [-0.6] * 1000)
    elif c["signal"] == "doc_split":
        x = np.array([0.01] * 2048 + [0.6] * 2048 + [-0.01] * 2048 + [0.5] * 2048)
    elif c["signal"] == "zeros":
        x = np.zeros(c["shape"])
    else:
        x = blocks(case_seed(name), c["shape"], c["frame_length"] + c["hop_length"], c["phase"])
    assert x.shape == c["shape"]
    return x.astype(c["dtype"])


def reference_arg(case):
    return np.max if case["reference"] == "max" else case["reference"]


def batches():
    """name -> (frame_length, hop_length, sweep case names): B = 1, 3 and 5 ragged rows per pair, length 1 beside the longest."""
    out = {}
    for fl, hop in PAIRS:
        names = ["sw_%d_%d_%d" % (fl, hop, n) for n in sweep_lengths(fl, hop)]
        longest = max(names, key=lambda k: SILENCE_CASES[k]["shape"][0])
        rest = [k for k in names if k not in (names[0], longest)]
        out["b1_%d_%d" % (fl, hop)] = (fl, hop, [longest])
        out["b3_%d_%d" % (fl, hop)] = (fl, hop, [names[0], longest, rest[-1]])
        out["b5_%d_%d" % (fl, hop)] = (fl, hop, [rest[0], longest, names[0], rest[-1], rest[len(rest) // 2]])
    return out


# ---- normalize ------------------------------------------------------------------------------------------------------------------------------
NORMS = ("max", "min", "mean", "mean_std", "l0", "l1", "l2")
EXACT_NORMS = ("max", "min", "l0")  # built from an order-free statistic: bit for bit
NORM_SHAPES = {"v5": (5,), "m4x3": (4, 3), "m3x1000": (3, 1000), "t2x3x257": (2, 3, 257), "z5": (5,)}
NORM_DTYPES = ("float32", "float64", "int64")


def normalize_input(name):
    """float64 noise in [-0.5, 0.5) with, for every axis, one line of exact zeros along it (the threshold branch); "z5": all zeros."""
    shape = NORM_SHAPES[name]
    if name == "z5":
        return np.zeros(shape)
    x = np.random.default_rng(case_seed(name)).random(shape) - 0.5
    if len(shape) > 1:
        for ax in range(len(shape)):
            idx = [0] * len(shape)
            idx[ax] = slice(None)
            x[tuple(idx)] = 0.0
    return x


def cast(x, dtype):
    return np.round(x * 1000).astype(np.int64) if dtype == "int64" else x.astype(dtype)


def kept(shape):
    """Flat positions of a result that the fixture stores: all of a small one, else every thirteenth with both ends."""
    size = int(np.prod(shape))
    if size <= 64:
        return np.arange(size)
    return np.unique(np.concatenate([np.arange(0, size, 13), np.arange(8), np.arange(size - 8, size)]))


def normalize_cases():
    for name, shape in NORM_SHAPES.items():
        for axis in range(len(shape)):
            for norm in NORMS:
                for dtype in NORM_DTYPES:
                    yield name, axis, norm, dtype


def norm_key(name, axis, norm, dtype):
    return "norm/%s/a%d/%s/%s" % (name, axis, norm, dtype)


def peak_error(y, ref):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(y, np.float64) - ref)
    peak = np.abs(ref).max() if ref.size else 0.0
    return float(err.max() / peak) if peak > 0 else float(err.max() if err.size else 0.0)


# ---- channels and indexing --------------------------------------------------------------------------------------------------------------------
MONO_CASES = {"mono_%s_c%d" % (dt, c): ((257, c) if c else (257,), dt) for dt in ("float32", "float64") for c in (0, 1, 2, 3, 8)}
MONO_CASES["mono_doc"] = ("doc", "float64")


def mono_input(name):
    shape, dtype = MONO_CASES[name]
    if shape == "doc":
        return np.array([[1, 2], [0.5, 0.1]])
    return (2.0 * np.random.default_rng(case_seed(name)).random(shape) - 1.0).astype(dtype)


_DOC3 = np.array([[1, 2, 3], [2, 3, 4], [3, 4, 5]])
_DOC10 = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10], [2, 3, 4, 5, 6, 7, 8, 9, 10, 11]])
_BG11 = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1]])
_V7 = np.arange(7, dtype=np.float32) - 2.5
_C3 = (np.arange(30, dtype=np.float64).reshape(10, 3) - 7.25) / 4
# name -> (function, arguments); every array argument is stored by the generator
INDEX_CASES = {
    "invert_doc": ("invert_channels", (_DOC3,)),
    "invert_1d": ("invert_channels", (_V7,)),
    "invert_c3": ("invert_channels", (_C3,)),
    "invert_c1": ("invert_channels", (_C3[:, :1].copy(),)),
    "loop_doc": ("loop", (_DOC3, 3)),
    "loop_1d": ("loop", (_V7, 2)),
    "loop_c3_once": ("loop", (_C3, 1)),
    "loop_c3_frac": ("loop", (_C3, 2.5)),
    "clip_doc": ("clip", (_DOC10, 0.1, 0.3)),
    "clip_1d": ("clip", (_V7, 0.3, 0.5)),
    "clip_c3": ("clip", (_C3, 0.2, 0.55)),
    "clip_out_of_range": ("clip", (_C3, 0.7, 0.5)),
    "insert_doc": ("insert_in_background", (_DOC10.T.copy(), 0.2, _BG11.T.copy())),
    "insert_1d": ("insert_in_background", (_V7, 0.5, np.arange(9, dtype=np.float32))),
    "insert_c3": ("insert_in_background", (_C3, 0.4, _C3[::-1].copy() * 2)),
    "insert_c3_mono_bg": ("insert_in_background", (_C3, 0.25, np.arange(8, dtype=np.float64))),
    "insert_1d_stereo_bg": ("insert_in_background", (_V7.astype(np.float64), 1.0, _C3[:, :2].copy())),
    "insert_out_of_range": ("insert_in_background", (_C3, 1.5, _C3)),
}
