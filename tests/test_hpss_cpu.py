"""CPU: what of data.features soft_mask / hpss / harmonic can be checked without a device - the fixture file against the case tables,
the median filter's window convention (the reference's recorded medians against a brute-force periodic-reflection median written
in hpss_cases.py), the public names and bound symbols, the refusals that come before any device call and the host-only paths of the
two new C entries."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import hpss_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return np.load(C.GOLDENS)


@pytest.fixture(scope="module")
def lib():
    from mindaudio_amd import _build, _lib

    _build.build()
    return _lib.load()


def test_fixture_is_current_with_the_case_tables(fix):
    assert os.path.getsize(C.GOLDENS) < os.path.getsize(os.path.join(HERE, "golden", "processing_goldens.npz"))
    want = set()
    for name, c in C.REAL_CASES.items():
        x = C.real_input(name)
        assert x.shape == c["shape"] and x.dtype == np.float32
        want.add("real/%s/sha" % name)
        assert str(fix["real/%s/sha" % name]) == C.sha(x), name  # the seeded input is the one the reference ran on
        if x.size <= C.STORE_INPUT_MAX:
            want.add("real/%s/x" % name)
            assert np.array_equal(fix["real/%s/x" % name], x) and fix["real/%s/x" % name].dtype == np.float32
        n_kept = len(C.kept(c["shape"]))
        for kernel, power, margin in C.real_runs(name):
            assert C.fits(kernel, c["shape"])
            for key in C.median_keys(name, kernel):
                want.add(key)
                assert fix[key].shape == c["shape"] and fix[key].dtype == np.uint8
            for label in ("mask_h", "mask_p", "out_h", "out_p"):
                key = "%s/%s" % (C.run_key(name, kernel, power, margin), label)
                want.add(key)
                assert fix[key].shape == (n_kept,) and fix[key].dtype == np.float32
    for dtype in C.SOFT_DTYPES:
        a, b = C.soft_mask_inputs(dtype)
        want |= {"soft/%s/a" % dtype, "soft/%s/b" % dtype}
        assert np.array_equal(fix["soft/%s/a" % dtype], a) and np.array_equal(fix["soft/%s/b" % dtype], b)
        for power in C.POWERS:
            for split_zeros in (False, True):
                key = C.soft_key(dtype, power, split_zeros)
                want.add(key)
                assert fix[key].shape == a.shape and fix[key].dtype == (np.bool_ if np.isinf(power) else np.dtype(dtype))
    for name in C.COMPLEX_SLICES:
        x = C.complex_input(name)
        want.add("complex/%s/sha" % name)
        assert str(fix["complex/%s/sha" % name]) == C.sha(x) and x.dtype == np.complex64
        mag = np.abs(x)
        assert ((mag == 0) | (mag >= C.MAG_FLOOR)).all()  # the condition on the fixtures
        for margin in C.COMPLEX_MARGINS:
            for label in ("mask_h", "mask_p", "out_h", "out_p"):
                key = "%s/%s" % (C.complex_key(name, margin), label)
                want.add(key)
                assert fix[key].shape == C.kept(C.COMPLEX_SHAPE).shape
                assert fix[key].dtype == (np.float32 if label.startswith("mask") else np.complex64)
    want |= {"harmonic/x", "harmonic/out", "harmonic/e32"}
    assert np.array_equal(fix["harmonic/x"], C.harmonic_input()) and fix["harmonic/out"].shape == (C.HARMONIC_N,)
    assert fix["harmonic/out"].dtype == np.float64 and fix["harmonic/e32"].shape == (2,)
    assert 0.0 < float(fix["harmonic/e32"][0]) < 2.0 ** -20 and 0.0 < float(fix["harmonic/e32"][1]) < 2.0 ** -20
    assert set(fix.files) == want


def test_the_cases_cover_what_the_kernels_branch_on():
    from mindaudio_amd import _lib
    from mindaudio_amd.data import features as F

    assert (C.SEGMENT, C.MAX_K) == (_lib.MEDIAN_SEGMENT, _lib.MEDIAN_MAX_K) == (F.MEDIAN_SEGMENT, F.MEDIAN_MAX_K)
    header = open(os.path.join(os.path.dirname(HERE), "include", "mindaudio_amd.h")).read()
    assert "#define MA_MEDIAN_SEGMENT %d\n" % C.SEGMENT in header and "#define MA_MEDIAN_MAX_K %d\n" % C.MAX_K in header
    shapes = [c["shape"] for c in C.REAL_CASES.values()]
    for axis in (-1, -2):  # an axis one shorter and one longer than a staged segment, more than one segment, and a short one
        lengths = {s[axis] for s in shapes}
        assert {C.SEGMENT - 1, C.SEGMENT + 1} <= lengths and max(lengths) > 2 * C.SEGMENT and min(lengths) < 16
    kernels = {k for c in C.REAL_CASES.values() for kernel in c["kernels"] for k in C.pair(kernel)}
    assert {1, 4, 17, 20, 31} <= kernels
    name, kernel = C.MULTI_REFLECTION
    assert kernel in C.REAL_CASES[name]["kernels"] and C.pair(kernel)[1] == 4 * C.REAL_CASES[name]["shape"][-2]  # k = 4n, the limit
    assert any(len(s) == 3 for s in shapes) and any(len(s) == 4 for s in shapes)
    assert {1, 2, 0.5, 3.7, np.inf} == set(C.POWERS)


def test_stored_medians_are_the_periodic_reflection_median(fix):
    """The convention of include/mindaudio_amd.h, pinned on the CPU: window i - k // 2 ... i - k // 2 + k - 1 (an even k leans left),
    rank k // 2 (the upper middle, no averaging), indices reflected d c b a | a b c d | d c b a periodically - against what the
    reference's scipy.ndimage.median_filter calls returned (decoded from their stored window offsets)."""
    assert np.array_equal(C.reflect_index(np.arange(-9, 12), 4), [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3])
    x = np.array([5.0, 1.0, 4.0, 2.0, 3.0], np.float32)
    assert np.array_equal(C.brute_median(x, 4, -1), [5, 5, 4, 3, 3])  # windows (1 5 5 1) (5 5 1 4) (5 1 4 2) (1 4 2 3) (4 2 3 3)
    assert np.array_equal(C.brute_median(x, 3, -1), [5, 4, 2, 3, 3])
    checked = set()
    for name, c in C.REAL_CASES.items():
        x = C.real_input(name)
        for kernel in c["kernels"]:
            for key, k, axis in zip(C.median_keys(name, kernel), C.pair(kernel), (-1, -2)):
                if key in checked:
                    continue
                checked.add(key)
                off = fix[key]
                assert off.max() < k
                ref = C.decode(x, off, k, axis)
                assert ref.dtype == np.float32 and np.array_equal(ref, C.brute_median(x, k, axis)), key
    assert len(checked) >= 20


def test_public_names_and_bound_symbols():
    from mindaudio_amd import _lib, data
    from mindaudio_amd.data import features as F

    for name in ("soft_mask", "hpss", "harmonic", "median_filter_device"):
        assert name in F.__all__ and callable(getattr(F, name)), name
    for name in ("soft_mask", "hpss", "harmonic"):
        assert getattr(data, name) is getattr(F, name)
    for sym in ("ma_median_filter", "ma_soft_mask"):
        assert sym in _lib.PROTOTYPES, sym
    assert len(_lib.PROTOTYPES["ma_median_filter"][1]) == 14 and len(_lib.PROTOTYPES["ma_soft_mask"][1]) == 14
    for name in ("resynthesize", "spectral_centroid", "complex_norm", "angle", "melscale"):  # not built
        assert not hasattr(F, name)


class _NoDevice:
    """Stands in for the module's device plumbing: any touch of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("a device call (%s) before the argument check" % name)


@pytest.fixture()
def no_device(monkeypatch):
    from mindaudio_amd.data import features as F

    monkeypatch.setattr(F, "_host", _NoDevice())
    return F


def test_refusals_come_before_any_device_call(no_device):
    F = no_device
    x = np.ones((5, 8), np.float32)
    with pytest.raises(TypeError, match="Margins must be >= 1.0"):
        F.hpss(x, margin=0.5)
    with pytest.raises(TypeError, match="Margins must be >= 1.0"):
        F.hpss(x, kernel_size=3, margin=(2.0, 0.99))
    with pytest.raises(TypeError, match="power must be strictly positive"):
        F.hpss(x, kernel_size=3, power=0)
    with pytest.raises(TypeError, match="shape mismatch"):
        F.soft_mask(x, x[:, :7])
    with pytest.raises(TypeError, match="power must be strictly positive"):
        F.soft_mask(x, x, power=0)
    with pytest.raises(TypeError, match="power must be strictly positive"):
        F.soft_mask(x, x, power=-1.5)
    # k > 4 n on either axis, and k > 127: ValueError naming both limits
    for kernel in (31, (31, 21), (33, 3), 128, (3, 128), 0):
        with pytest.raises(ValueError, match=r"<= 127 and size <= 4 \* axis length"):
            F.hpss(np.ones((5, 8) if kernel != 128 and kernel != (3, 128) else (64, 64), np.float32), kernel_size=kernel)
    with pytest.raises(ValueError):
        F.hpss(np.ones(8, np.float32))


def test_new_entries_reject_bad_arguments_without_a_gpu(lib):
    from mindaudio_amd import _lib

    buf = (ctypes.c_double * 64)()  # host memory: every call below must return before it could be touched
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    q = ctypes.cast(ctypes.addressof(buf) + 256, ctypes.c_void_p)

    def mf(x=p, dtype=0, rows=1, n=8, inner=4, xs=(32, 4, 1), k=5, out=q, os_=(32, 4, 1)):
        return lib.ma_median_filter(x, dtype, rows, n, inner, xs[0], xs[1], xs[2], k, out, os_[0], os_[1], os_[2], null)

    for bad in (dict(x=null), dict(out=null), dict(out=p), dict(dtype=2), dict(dtype=-1), dict(rows=0), dict(n=0), dict(inner=0), dict(k=0),
                dict(k=-3), dict(k=33), dict(k=128), dict(n=40, k=128), dict(xs=(32, -4, 1)), dict(os_=(-1, 4, 1))):
        assert mf(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    assert mf(n=2, k=9) == _lib.MA_ERR_INVALID_ARG  # k <= 4 n
    assert mf(rows=2 ** 31, n=2 ** 20) == _lib.MA_ERR_UNSUPPORTED
    assert mf(rows=2 ** 20, n=2 ** 20, inner=2 ** 20) == _lib.MA_ERR_UNSUPPORTED

    def sm(a=p, b=p, dtype=0, count=8, power=2.0, mask=q, spec=null, phase=null, out=null):
        return lib.ma_soft_mask(a, b, dtype, count, 1.0, 1.0, power, 0, mask, spec, phase, out, null, null)

    for bad in (dict(a=null), dict(b=null), dict(dtype=3), dict(count=0), dict(power=0.0), dict(power=-1.0), dict(power=float("nan")),
                dict(mask=null), dict(out=q), dict(mask=null, phase=p, spec=p), dict(dtype=1, spec=p, phase=p, out=q)):
        assert sm(**bad) == _lib.MA_ERR_INVALID_ARG, bad
    assert sm(count=2 ** 40) == _lib.MA_ERR_UNSUPPORTED
