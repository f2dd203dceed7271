"""CPU: what of data.processing's silence front end, normalize, stereo_to_mono and indexing functions can be checked without a
device - the fixture file against the case tables, the public names, the refusals that come before any device call, the host-only
paths of the new C entries, and the host form of the boundary logic against the reference's indices on the stored flags."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import processing_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return np.load(C.GOLDENS)


@pytest.fixture(scope="module")
def lib():
    from mindaudio_amd import _build, _lib

    _build.build()
    return _lib.load()


def test_fixture_is_current_with_the_case_tables(fix):
    assert os.path.getsize(C.GOLDENS) < (1 << 20)
    want = {"smallest_margin"}
    for name, c in C.SILENCE_CASES.items():
        want |= {name + "/" + k for k in ("x", "power", "db", "flags", "margin", "split")}
        assert (name + "/trim_index" in fix.files) != (name + "/trim_error" in fix.files), name
        want.add(name + ("/trim_index" if name + "/trim_index" in fix.files else "/trim_error"))
        x = fix[name + "/x"]
        assert x.shape == c["shape"] and x.dtype == np.dtype(c["dtype"]) and np.array_equal(x, C.silence_signal(name)), name
        F = C.num_frames(c["shape"][0], c["frame_length"], c["hop_length"])
        assert fix[name + "/power"].shape == fix[name + "/db"].shape == fix[name + "/flags"].shape == (F,)
        assert np.array_equal(fix[name + "/flags"], fix[name + "/db"] > -c["top_db"])
        margin = float(fix[name + "/margin"])
        assert margin == np.abs(fix[name + "/db"] + c["top_db"]).min() and margin >= C.MARGIN_DB, name  # the condition on the fixtures
    assert float(fix["smallest_margin"]) == min(float(fix[n + "/margin"]) for n in C.SILENCE_CASES)
    assert str(fix[C.NONE_PASS_CASE + "/trim_error"]) == "IndexError" and fix[C.NONE_PASS_CASE + "/split"].shape == (0, 2)
    for name in C.NORM_SHAPES:
        want.add("norm/%s/x" % name)
        assert np.array_equal(fix["norm/%s/x" % name], C.normalize_input(name))
    for name, axis, norm, dtype in C.normalize_cases():
        key = C.norm_key(name, axis, norm, dtype)
        want.add(key)
        assert fix[key].shape == C.kept(C.NORM_SHAPES[name]).shape
        assert fix[key].dtype == (np.float64 if norm in ("mean", "mean_std") else np.dtype(dtype)), key
        if norm not in C.EXACT_NORMS:
            want.add(key + "/spread")
            assert 0.0 <= float(fix[key + "/spread"]) < 2.0 ** -40
    for name in C.MONO_CASES:
        want |= {name + "/x", name + "/out"}
        assert np.array_equal(fix[name + "/x"], C.mono_input(name))
    for name, (fn, args) in C.INDEX_CASES.items():
        want |= {name + "/out", name + "/printed"}
        for k, a in enumerate(args):
            if isinstance(a, np.ndarray):
                want.add("%s/arg%d" % (name, k))
                assert np.array_equal(fix["%s/arg%d" % (name, k)], a) and fix["%s/arg%d" % (name, k)].dtype == a.dtype
    assert set(fix.files) == want


def test_the_cases_cover_what_the_kernels_branch_on():
    from mindaudio_amd import _lib

    assert (C.TILE, C.MAX_RATIO) == (_lib.FRAME_POWER_TILE, _lib.FRAME_POWER_MAX_RATIO)
    header = open(os.path.join(os.path.dirname(HERE), "include", "mindaudio_amd.h")).read()
    assert "#define MA_FRAME_POWER_TILE %d\n" % C.TILE in header and "#define MA_FRAME_POWER_MAX_RATIO %d\n" % C.MAX_RATIO in header
    assert "#define MA_CHANNEL_MEAN_MAX %d\n" % _lib.CHANNEL_MEAN_MAX in header
    ratios = {fl // hop if fl % hop == 0 else 0 for fl, hop in C.PAIRS}
    assert {0, 1, C.MAX_RATIO, C.MAX_RATIO + 1} <= ratios  # direct sums, one block, the last ratio with block sums, the first without
    for fl, hop in C.PAIRS:
        frames = [C.num_frames(n, fl, hop) for n in C.sweep_lengths(fl, hop)]
        assert 1 in frames and C.TILE + 1 in frames  # one frame, and one frame into the second tile
    assert any(fl % 2 for fl, _ in C.PAIRS) and any(hop > fl for fl, hop in C.PAIRS)


def test_public_names():
    from mindaudio_amd.data import processing as P

    for name in ("normalize", "unitarize", "resample", "rescale", "stereo_to_mono", "trim", "split", "invert_channels", "loop", "clip",
                 "insert_in_background", "frame_power_device", "trim_batch", "split_batch"):
        assert name in P.__all__ and callable(getattr(P, name)), name
    for name in ("sliding_window_cmn", "overlap_and_add"):  # not built, and said so
        assert name not in P.__all__ and not hasattr(P, name) and name in P.__doc__


class _NoDevice:
    """Stands in for the module's device plumbing: any touch of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("a device call (%s) before the argument check" % name)


@pytest.fixture()
def no_device(monkeypatch):
    from mindaudio_amd.data import processing as P

    monkeypatch.setattr(P, "_host", _NoDevice())
    return P


def test_refusals_come_before_any_device_call(no_device):
    P = no_device
    x = np.zeros((8, 2), np.float32)
    with pytest.raises(TypeError):
        P.normalize(x, norm="rms")
    with pytest.raises(NotImplementedError):
        P.normalize(x.astype(np.complex128))
    with pytest.raises(NotImplementedError):
        P.normalize(x, axis=(0, 1))
    with pytest.raises(ValueError):
        P.normalize(x, axis=2)
    with pytest.raises(IndexError):  # (np.exceptions.AxisError is both)
        P.normalize(x, axis=-3)
    with pytest.raises(NotImplementedError):
        P.stereo_to_mono(np.zeros((4, 9), np.float32))
    with pytest.raises(NotImplementedError):
        P.stereo_to_mono(x.astype(np.complex64))
    for fn in (P.trim, P.split):
        with pytest.raises(ValueError):
            fn(x, hop_length=0)
        with pytest.raises(ValueError):
            fn(x, frame_length=0)
        with pytest.raises(ValueError):
            fn(np.zeros((2, 3, 4), np.float32))
        with pytest.raises(NotImplementedError):
            fn(x.astype(np.complex64))
    with pytest.raises(NotImplementedError):
        P.insert_in_background(x, 0.5, None)
    v = np.arange(5.0)
    assert P.stereo_to_mono(v) is v and P.invert_channels(v) is v and P.loop(v, 1) is v and P.loop(v, 0.5) is v
    with contextlib.redirect_stdout(io.StringIO()) as said:
        assert P.clip(v, 0.8, 0.4) is v and P.insert_in_background(v, -0.1, v) is v
    assert said.getvalue() == "Combination of offset and duration factors exceed audio length.\nOffset factor number exceed range [0, 1].\n"


def test_indexing_functions_on_numpy_need_no_device(no_device, fix):
    P = no_device
    for name, (fn, args) in C.INDEX_CASES.items():
        call = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
        with contextlib.redirect_stdout(io.StringIO()) as said:
            y = getattr(P, fn)(*call)
        ref = fix[name + "/out"]
        assert said.getvalue() == str(fix[name + "/printed"])
        assert y.dtype == ref.dtype and y.shape == ref.shape and np.array_equal(y, ref), name
        for a, b in zip(call, args):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b), name  # nothing is overwritten


def test_new_entries_reject_bad_arguments_without_a_gpu(lib):
    from mindaudio_amd import _lib

    assert lib.ma_frame_power_frames(3000, 2048, 512) == 6 and lib.ma_frame_power_frames(8192, 2048, 512) == 17
    for fl, hop in C.PAIRS:
        for n in C.sweep_lengths(fl, hop):
            assert lib.ma_frame_power_frames(n, fl, hop) == C.num_frames(n, fl, hop)
    assert lib.ma_frame_power_frames(3, 7, 3) == 1 and lib.ma_frame_power_frames(4, 7, 3) == 2  # odd frame_length: (n - 1) // hop + 1
    for bad in ((0, 64, 16), (10, 0, 16), (10, 64, 0)):
        assert lib.ma_frame_power_frames(*bad) == _lib.MA_ERR_INVALID_ARG
    buf = (ctypes.c_double * 64)()  # host memory: every call below must return before it could be touched
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)

    def fp(x=p, sample_bytes=4, B=1, T=32, ldx=32, fl=8, hop=4, power=p, ldp=9, row_max=p):
        return lib.ma_frame_power(x, sample_bytes, B, T, ldx, null, fl, hop, power, ldp, row_max, null)

    def se(power=p, ldp=9, B=1, T=32, fl=8, hop=4, clip=-1, flags=p, index=p, counts=p, edges=p):
        return lib.ma_silence_edges(power, ldp, B, T, null, fl, hop, null, 1.0, 60.0, clip, flags, index, counts, edges, null)

    for bad in (dict(x=null), dict(power=null), dict(row_max=null), dict(sample_bytes=2), dict(B=0), dict(T=0), dict(fl=0), dict(hop=0),
                dict(fl=-1), dict(hop=-3), dict(ldx=31), dict(ldp=8)):
        assert fp(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    assert fp(T=2 ** 31, ldx=2 ** 31, ldp=2 ** 29 + 1) == _lib.MA_ERR_UNSUPPORTED
    for bad in (dict(power=null), dict(flags=null), dict(index=null), dict(counts=null), dict(edges=null), dict(B=0), dict(T=0),
                dict(fl=0), dict(hop=0), dict(ldp=8), dict(clip=2 ** 31)):
        assert se(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    for bad in ((null, 0, 1, 4, 1, 0, p), (p, 0, 1, 4, 1, 0, null), (p, 4, 1, 4, 1, 0, p), (p, -1, 1, 4, 1, 0, p), (p, 0, 0, 4, 1, 0, p),
                (p, 0, 1, 0, 1, 0, p), (p, 0, 1, 4, 0, 0, p), (p, 0, 1, 4, 1, 7, p), (p, 0, 1, 4, 1, -1, p)):
        assert lib.ma_axis_stats(*bad, null) == _lib.MA_ERR_INVALID_ARG, bad
    q = ctypes.cast(ctypes.addressof(buf) + 256, ctypes.c_void_p)
    for bad in ((null, 0, 1, 4, 1, p, p, q, 0), (p, 0, 1, 4, 1, p, p, null, 0), (p, 0, 1, 4, 1, null, null, q, 0), (p, 0, 1, 4, 1, p, p, p, 0),
                (p, 4, 1, 4, 1, p, p, q, 1), (p, 0, 1, 4, 1, p, p, q, 2), (p, 3, 1, 4, 1, p, p, q, 0), (p, 0, 0, 4, 1, p, p, q, 0),
                (p, 0, 1, 0, 1, p, p, q, 0), (p, 0, 1, 4, 0, p, p, q, 0)):
        assert lib.ma_axis_apply(*bad, null) == _lib.MA_ERR_INVALID_ARG, bad
    for bad in ((null, 4, 4, 2, p), (p, 4, 4, 2, null), (p, 2, 4, 2, p), (p, 4, 0, 2, p), (p, 4, 4, 0, p)):
        assert lib.ma_channel_mean(*bad, null) == _lib.MA_ERR_INVALID_ARG, bad
    assert lib.ma_channel_mean(p, 4, 4, _lib.CHANNEL_MEAN_MAX + 1, p, null) == _lib.MA_ERR_UNSUPPORTED


def test_host_edge_logic_matches_the_reference_on_the_stored_flags(fix):
    from mindaudio_amd.data import processing as P

    for name, c in C.SILENCE_CASES.items():
        index, bounds = P.host_edges(fix[name + "/flags"], c["hop_length"])
        if name + "/trim_error" in fix.files:
            assert index is None and bounds.size == 0
        else:
            assert np.array_equal(index, fix[name + "/trim_index"]), name
        assert np.array_equal(np.minimum(bounds, c["shape"][-1]).reshape(-1, 2), fix[name + "/split"]), name
        assert P.num_frames(c["shape"][0], c["frame_length"], c["hop_length"]) == len(fix[name + "/flags"])


def test_channel_order_is_numpys(fix):
    """The order ma_channel_mean adds in, written out in NumPy: index order below eight channels, the pairs of add.reduce's unrolled
    block at eight.  If a NumPy release changes its order, this fails here rather than on the device."""
    for name, (shape, dtype) in C.MONO_CASES.items():
        x = fix[name + "/x"]
        if x.ndim < 2:
            continue
        ch = [x[:, k] for k in range(x.shape[1])]
        if len(ch) == 8:
            acc = ((ch[0] + ch[1]) + (ch[2] + ch[3])) + ((ch[4] + ch[5]) + (ch[6] + ch[7]))
        else:
            acc = ch[0]
            for k in range(1, len(ch)):
                acc = acc + ch[k]
        y = acc / x.dtype.type(len(ch))
        assert y.dtype == x.dtype and np.array_equal(y, fix[name + "/out"]) and np.array_equal(y, np.mean(x, axis=-1)), name
